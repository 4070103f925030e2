from efficient_gnns_amd.nn import GATConv, GCNConv, MessagePassing, SAGEConv  # noqa: F401
