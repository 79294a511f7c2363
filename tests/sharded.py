"""What the multi-rank tests share (a helper module, not a conftest): which rank owns a separator's panel, the factor assembled from the ranks'
arenas, and the gather of the factor onto rank 0."""
import numpy as np


def panel_owners(plan, world):
    """{separator label: the rank whose subtree holds it}; the separators above the cut (the shared top, complete on every rank) count as rank 0's."""
    d = world.bit_length() - 1
    tree = plan.tree
    owner = {}
    for h in range(1, plan.nsep + 1):
        lvl = h.bit_length() - 1
        owner[int(tree[h - 1])] = 0 if lvl < d else (h >> (lvl - d)) - (1 << d)
    return owner


def panel_ranges(plan):
    """{separator label: (first, end) arena element of its panel}: a panel runs from its diagonal block to the next panel's."""
    diag = {int(b[1]): int(b[7]) for b in plan.blocks if b[0] == b[1]}
    order = sorted(diag)
    return {s: (diag[s], diag[order[i + 1]] if i + 1 < len(order) else plan.arena_doubles) for i, s in enumerate(order)}


def assemble(plan, parts, world, ref_like=None):
    """Panel of separator s from its owner's arena, the top from rank 0 (`parts`: the ranks' arenas as host arrays)."""
    owner = panel_owners(plan, world)
    out = np.zeros_like(parts[0] if ref_like is None else ref_like)
    for s, (lo, hi) in panel_ranges(plan).items():
        out[lo:hi] = parts[owner[s]][lo:hi]
    return out


def gather_factor(devs, arenas, f32=False):
    """cholamd_gather_factor / _f32 over the rank objects of one process: arenas[0] then holds the complete factor."""
    import ctypes as C
    from cholesky_amd import _lib
    n = len(devs)
    hd = (C.c_void_p * n)(*[d.h for d in devs])
    ha = (C.c_void_p * n)(*[C.c_void_p(a.data_ptr()) for a in arenas])
    L = devs[0].L
    _lib.check((L.cholamd_gather_factor_f32 if f32 else L.cholamd_gather_factor)(hd, ha, n, None), "cholamd_gather_factor")
    devs[0].sync()
