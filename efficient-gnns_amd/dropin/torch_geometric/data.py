"""``torch_geometric.data`` names of the reference's MAG script (/root/reference/mag_pyg/gnn.py:15) and of graph-level batches."""
from efficient_gnns_amd.saint import Batch, Data, GraphSAINTRandomWalkSampler  # noqa: F401
