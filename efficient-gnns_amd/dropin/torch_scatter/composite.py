"""``torch_scatter.composite``: the softmax family of the shim (``from torch_scatter.composite import scatter_softmax``)."""
from . import scatter_log_softmax, scatter_softmax  # noqa: F401
