"""Reading the per-view kernels of a golden ``rl_*.npz`` (numpy only: the JNA child
imports this too).

A file whose views share one kernel size stacks them: ``psfs``, ``k1`` and ``k2`` are
[view, z, y, x].  A file with per-view sizes (``rl_mixed_ksize``) cannot: each kernel
sits in the low corner of a zero frame of the largest dims, and ``kdims`` [view, 3] holds
its own (z, y, x) dims, which the kernel preparation and the session must be given.
"""
import numpy as np


def kernels(g, name):
    """The list of view kernels ``name`` ('psfs', 'k1' or 'k2') of the loaded file ``g``,
    each in its own dims."""
    a = g[name]
    if "kdims" not in g.files:
        return list(a)
    return [np.ascontiguousarray(k[:d[0], :d[1], :d[2]]) for k, d in zip(a, g["kdims"])]


def stack(ks):
    """The inverse: kernels of any dims in the low corner of one zero frame."""
    big = [max(k.shape[d] for k in ks) for d in range(3)]
    out = np.zeros([len(ks)] + big, np.float32)
    for v, k in enumerate(ks):
        out[v, :k.shape[0], :k.shape[1], :k.shape[2]] = k
    return out
