"""``torch_geometric.data`` names of the reference's MAG script (/root/reference/mag_pyg/gnn.py:15)."""
from efficient_gnns_amd.saint import Data, GraphSAINTRandomWalkSampler  # noqa: F401
