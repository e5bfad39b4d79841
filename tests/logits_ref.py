"""z = Why*h + by as the inference heads sum it (k_gen_head, k_code_head; DESIGN.md sections 3.5 and 3.6): one thread per
logit, sequentially in k, with a separate float32 multiply and add.  Shared by tests/test_logit_processors.py and the
coder's table tests."""
import numpy as np

M = 256
f32 = np.float32


def logits32(Why, by, h):
    """Why [256, N], by [256], h [N] (float32): the 256 logits"""
    z = np.zeros(M, f32)
    for k in range(h.size):
        z = (z + (Why[:, k] * h[k]).astype(f32)).astype(f32)
    return (z + by).astype(f32)
