"""x265_amd — MI355X (gfx950) batched backend for the x265 1.9 primitive table.

The product is the C-ABI shared library libx265amd.so (include/x265_amd.h)
built from csrc/*.hip; this package only builds and binds it.
"""
from .native import (LIB_PATH, InterBest, InterCostBatch, IntraBest, IntraCostBatch, Primitives,  # noqa: F401
                     X265AmdError, capture_graph, inter_cost_batches, intra_cost_batches)
