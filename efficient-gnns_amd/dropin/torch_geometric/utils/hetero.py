"""``torch_geometric.utils.hetero`` name of the reference's MAG script (/root/reference/mag_pyg/gnn.py:16)."""
from efficient_gnns_amd.utils import group_hetero_graph  # noqa: F401
