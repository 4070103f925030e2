from efficient_gnns_amd.nn import GATConv, GCNConv, MessagePassing, SAGEConv  # noqa: F401
from efficient_gnns_amd.nn import GINConv, GINEConv, global_add_pool, global_max_pool, global_mean_pool  # noqa: F401
