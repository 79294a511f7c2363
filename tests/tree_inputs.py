"""Synthetic elimination trees for the factor and solve tests (a helper module, not a conftest).

Every other input of the suite is a grid: its separators are planes of a box, so their sizes are a handful of products and a leaf, its parent and
its grandparent always come in the same ratios.  A tree input names the size of every separator, so a pivot of exactly 145, 177, 193, 257 or 273
columns can be a leaf, a middle separator or a root.  A spec is a dict:

  levels     1 .. 7 (the separator file holds one digit)
  sizes      one size >= 1 per node of the complete binary tree in heap order (root first; label of heap index h = nsep - (h - 1))
  tile       interval-0 cluster tiles of about `tile` dofs as the generator cuts them, or "random": a seeded strictly increasing boundary list with
             1-dof tiles that is not aligned to 16.  A separator at tree level l has the intervals 0 .. max(0, levels - 2 - l), later intervals
             index the list before them and the last one is a single tile -- what chol_symbolic.c requires
  leaf       internal pattern of the leaves, cycled in heap order: ("band", w) | "dense" | ("random", p) | "arrow" (a chain plus 16 dense last rows)
  inner      internal pattern of the other separators, cycled: "dense" | ("random", p)
  coupling   pattern of the block (ancestor r, separator c), cycled over the pairs in the order c = 2, 3, ...; r = parent, grandparent, ...:
             "dense" | ("random", p) | "tiles" | ("rows", m) | "none".  ("rows", m): the first m rows of r, all columns of c.  "tiles": only a
             seeded subset of r's 16-row tiles is touched, all columns of c, and the two children of a node take disjoint subsets (row
             compaction, block_tile_map).  "none" applies above the parent only; for the parent the next kind of the cycle is taken
  seed       of the permutation, the boundaries and the patterns (the values have the seed of spd_inputs.SPD)

An entry couples a separator with itself or with an ancestor only, so the ordering drops nothing (plan.dropped == 0).  `build()` writes the separator
and cluster files in the reference's formats and returns the pattern in original dof ids; spd_inputs.SPD takes a spec as its `base`, draws the values
as for every other input, writes the matrix file and makes the plan from the three files, so the readers see files no grid produced.  It also
builds the plan from the same arrays (Plan.from_arrays) and holds the two equal."""
import os

import numpy as np

SWEEP_SIZES = [1, 15, 16, 17, 63, 64, 65, 127, 128, 129, 143, 144, 145, 159, 160, 161, 175, 176, 177, 191, 192, 193, 255, 256, 257, 271, 272, 273,
               287, 288, 289, 511, 512, 513]

def _deep_sizes():
    """tree_deep: 80, 40, 33 on the top two levels, 60 separators of 3 .. 7 columns below them and 64 leaves of 16 .. 21 (n = 1634)."""
    rng = np.random.default_rng(3)
    return [80, 40, 33] + [int(v) for v in rng.integers(3, 8, 60)] + [int(v) for v in rng.integers(16, 22, 64)]


def _deep_coupling():
    """tree_deep: dense, dense, ("random", 0.5) cycled over the pairs (so every separator reaches every ancestor), but every fourth leaf touches
    the first 48 rows of the root only: the root's tile pairs inside those rows collect a source from each of the 64 leaves, the others from 48."""
    cycle, out = ["dense", "dense", ("random", 0.5)], []
    for c in range(2, 128):
        r = c // 2
        while r >= 1:
            out.append(("rows", 48) if c >= 64 and c % 4 == 3 and r == 1 else cycle[len(out) % 3])
            r //= 2
    return out


# the named trees: the first four join spd_inputs.INPUTS, the others are single-purpose
TREES = {
    "tree_over": dict(levels=3, sizes=[193, 177, 145, 257, 273, 17, 1], tile=32, leaf=[("band", 17), "dense", ("random", 0.3), "dense"],
                      inner=["dense", ("random", 0.5)], coupling=["dense", "tiles", "tiles"], seed=11),
    "tree_at": dict(levels=3, sizes=[192, 176, 144, 256, 272, 16, 15], tile=48, leaf=[("band", 17), "dense", ("random", 0.3), "dense"],
                    inner=["dense", ("random", 0.5)], coupling=["dense", "tiles", "tiles"], seed=12),
    "tree_skew": dict(levels=4, sizes=[161, 1, 160, 1, 1, 129, 128, 1, 1, 1, 1, 289, 1, 63, 65], tile="random",
                      leaf=["dense", ("band", 64), "arrow", ("band", 65), ("band", 80), ("random", 0.2), ("band", 15), ("band", 16)],
                      inner=["dense", ("random", 0.5)], coupling=["tiles", "none", "tiles", ("random", 0.3)], seed=13),
    "tree_tiny": dict(levels=4, sizes=[1, 2, 3, 1, 1, 5, 7, 1, 1, 1, 1, 31, 33, 1, 2], tile=4,
                      leaf=["dense", ("band", 1), "arrow", ("random", 0.5)], inner=["dense", ("random", 0.5)],
                      coupling=["dense", ("random", 0.4), "none", "tiles"], seed=14),
    "tree_single": dict(levels=1, sizes=[300], tile=32, leaf=[("random", 0.2)], inner=["dense"], coupling=["dense"], seed=15),
    "tree_two": dict(levels=2, sizes=[129, 65, 127], tile=32, leaf=[("band", 17), "arrow"], inner=["dense"], coupling=[("random", 0.3)], seed=16),
    # top separators of more than two column blocks (433 = 112 + 112 + 112 + 97, 289 = 112 + 112 + 65) next to one of a single column: under the
    # distributed top the cyclic owner rule (block + heap index) mod world wraps, a super-block of three column blocks ends inside the root and
    # at world 2 a rank owns two blocks of one separator that are not neighbours
    "tree_top": dict(levels=3, sizes=[433, 289, 1, 65, 17, 33, 129], tile="random",
                     leaf=["dense", ("band", 17), "arrow", ("random", 0.3)], inner=["dense", ("random", 0.5)],
                     coupling=["tiles", "dense", ("random", 0.3)], seed=17),
    # seven levels with dense couplings to every ancestor: a 64 x 64 target tile of the upper separators collects a source from each descendant, so
    # the macro-tile update kernels read their source descriptors in more than one batch of 32 (tests/test_update_mt_host.py counts them)
    "tree_deep": dict(levels=7, sizes=_deep_sizes(), tile=16, leaf=["dense", ("band", 5)], inner=["dense"], coupling=_deep_coupling(), seed=80),
}
NAMED = ["tree_over", "tree_at", "tree_skew", "tree_tiny"]
SINGLE = ["tree_single", "tree_two"]
DEEP = ["tree_deep"]                                     # the macro-tile update tests' own input (tests/test_gpu_update_mt.py)
TOP = ["tree_top"]                                       # the multi-rank tests' own input (tests/test_gpu_sharded_general.py)
WITH_TILES = ["tree_over", "tree_at", "tree_skew"]       # "tiles" couplings above the parent with more than one 16-row tile to choose from


def sweep_spec(position, s, leaf="dense"):
    """A 3-level tree with `s` columns at `position` ("leaf", "middle", "root") and small fixed odd sizes elsewhere (n = s + 142)."""
    sizes = {"leaf": [33, 17, 5, s, 29, 21, 37], "middle": [33, s, 17, 5, 21, 29, 37], "root": [s, 33, 17, 5, 29, 21, 37]}[position]
    return dict(levels=3, sizes=sizes, tile=16, leaf=[leaf if position == "leaf" else "dense", ("band", 5), ("random", 0.4), "arrow"],
                inner=["dense", "dense", ("random", 0.5)], coupling=["dense", "tiles", ("random", 0.4)], seed=100 + s)


def _internal(kind, m, rng):
    """Strictly lower (i, j) of one separator's own block, local indices."""
    i, j = np.tril_indices(m, -1)
    if kind == "dense":
        keep = np.ones(len(i), dtype=bool)
    elif kind == "arrow":
        keep = (i - j == 1) | (i >= m - 16)
    elif kind[0] == "band":
        keep = i - j <= kind[1]
    else:
        assert kind[0] == "random", kind
        keep = rng.random(len(i)) < kind[1]
    return i[keep], j[keep]


def _tile_subsets(ntiles, rng):
    """Disjoint subsets of an ancestor's 16-row tiles for the two children of a node (one tile: both take it)."""
    order = rng.permutation(ntiles)
    k = max(1, ntiles // 3)
    return (order[:k], order[k:2 * k]) if ntiles >= 2 * k and ntiles > 1 else (order[:k], order[-k:])


def _boundaries(spec, size, need, rng):
    """The boundary lists of one separator, intervals 0 .. need (the last one a single tile)."""
    lists, units = [], size
    for t in range(need + 1):
        if t == need:
            b = np.array([0, units])
        elif spec["tile"] == "random":
            if t == 0:
                k = min(units - 1, max(1, units // 24))
                inner = set(rng.choice(np.arange(1, units), size=k, replace=False).tolist()) if units > 1 else set()
                if units >= 3:                          # a 1-dof tile; one of q, q + 1 is no multiple of 16
                    q = int(rng.integers(1, units - 1))
                    inner |= {q, q + 1}
            else:
                k = int(rng.integers(0, max(1, (units - 1) // 2) + 1)) if units > 1 else 0
                inner = set(rng.choice(np.arange(1, units), size=min(k, units - 1), replace=False).tolist()) if units > 1 else set()
            b = np.array(sorted({0, units} | inner))
        else:
            m = max(1, -(-units // spec["tile"])) if t == 0 else max(1, (units + 1) // 2)
            m = min(m, units)
            b = np.array([units * q // m for q in range(m + 1)])
        assert b[0] == 0 and b[-1] == units and (np.diff(b) > 0).all()
        lists.append(b)
        units = len(b) - 1
    return lists


class Tree:
    """The arrays of one spec: perm, sep_sizes (by label), the cluster triples, the strictly-lower pattern in original dof ids, and where the
    "tiles" couplings left 16-row tiles of an ancestor untouched."""

    def __init__(self, spec):
        levels, sizes = spec["levels"], list(spec["sizes"])
        ns = (1 << levels) - 1
        assert 1 <= levels <= 7 and len(sizes) == ns and min(sizes) >= 1
        rng = np.random.default_rng(spec["seed"])
        self.levels, self.nsep, self.n = levels, ns, int(sum(sizes))
        self.heap_sizes = sizes
        self.sep_sizes = np.array([sizes[ns - lbl] for lbl in range(1, ns + 1)], dtype=np.int32)          # label -> heap index ns - label + 1
        off_lbl = np.concatenate([[0], np.cumsum(self.sep_sizes)])
        self.offset = {h: int(off_lbl[ns - h]) for h in range(1, ns + 1)}                                  # heap index -> first permuted position
        self.perm = rng.permutation(self.n).astype(np.int32)
        # clusters
        idx, itv, sep = [], [], []
        self.boundaries = {}
        for lbl in range(1, ns + 1):
            h = ns - lbl + 1
            need = max(0, levels - 2 - (h.bit_length() - 1))
            self.boundaries[h] = _boundaries(spec, sizes[h - 1], need, rng)
            for t, b in enumerate(self.boundaries[h]):
                idx += b.tolist()
                itv += [t] * len(b)
                sep += [lbl] * len(b)
        self.cl_idx, self.cl_interval, self.cl_sep = (np.array(a, dtype=np.int32) for a in (idx, itv, sep))
        # pattern, permuted positions
        rows, cols = [], []
        n_leaf = n_inner = n_pair = 0
        self.kinds, self.untouched_tiles = {}, 0
        subsets = {}
        for h in range(1, ns + 1):
            if h.bit_length() == levels:
                kind = spec["leaf"][n_leaf % len(spec["leaf"])]
                n_leaf += 1
            else:
                kind = spec["inner"][n_inner % len(spec["inner"])]
                n_inner += 1
            self.kinds[h, h] = kind
            i, j = _internal(kind, sizes[h - 1], rng)
            rows.append(self.offset[h] + i)
            cols.append(self.offset[h] + j)
        for c in range(2, ns + 1):
            r = c // 2
            while r >= 1:
                kind = spec["coupling"][n_pair % len(spec["coupling"])]
                n_pair += 1
                if kind == "none" and r == c // 2:
                    kind = spec["coupling"][n_pair % len(spec["coupling"])]
                    n_pair += 1
                    assert kind != "none"
                self.kinds[r, c] = kind
                mr, mc = sizes[r - 1], sizes[c - 1]
                if kind == "none":
                    keep = np.zeros((mr, mc), dtype=bool)
                elif kind == "dense":
                    keep = np.ones((mr, mc), dtype=bool)
                elif kind == "tiles":
                    nt = (mr + 15) // 16
                    if (r, c & ~1) not in subsets:
                        subsets[r, c & ~1] = _tile_subsets(nt, rng)
                    mine = subsets[r, c & ~1][c & 1]
                    keep = np.zeros((mr, mc), dtype=bool)
                    keep[np.isin(np.arange(mr) // 16, mine), :] = True
                    self.untouched_tiles += nt - len(mine)
                elif kind[0] == "rows":
                    keep = np.zeros((mr, mc), dtype=bool)
                    keep[:kind[1], :] = True
                else:
                    assert kind[0] == "random", kind
                    keep = rng.random((mr, mc)) < kind[1]
                    if not keep.any():
                        keep[rng.integers(mr), rng.integers(mc)] = True
                i, j = np.nonzero(keep)
                rows.append(self.offset[r] + i)
                cols.append(self.offset[c] + j)
                r //= 2
        pi, pj = np.concatenate(rows), np.concatenate(cols)
        assert (pi > pj).all()
        a, b = self.perm[pi].astype(np.int64), self.perm[pj].astype(np.int64)
        self.lo, self.hi = np.maximum(a, b), np.minimum(a, b)

    def write(self, prefix):
        """<prefix>_ord_<levels>.txt and <prefix>_clust_<levels>.txt."""
        lv, ns = self.levels, self.nsep
        ordf, clustf = f"{prefix}_ord_{lv}.txt", f"{prefix}_clust_{lv}.txt"
        off = np.concatenate([[0], np.cumsum(self.sep_sizes)])
        with open(ordf, "w") as f:
            f.write(f"{lv} {ns}\n")
            for lbl in range(1, ns + 1):
                f.write(f"{lbl - 1};" + "".join(f"{d}," for d in self.perm[off[lbl - 1]:off[lbl]]) + "\n")
        with open(clustf, "w") as f:
            f.write(f"{lv} {ns}\n")
            for lbl in range(1, ns + 1):
                lists = self.boundaries[ns - lbl + 1]
                f.write(f"{lbl - 1};" + ";".join("".join(f"{v}," for v in b) for b in lists) + ";\n")
        return ordf, clustf

    def plan_from_arrays(self, row, col, val):
        import cholesky_amd as ca
        return ca.Plan.from_arrays(self.n, self.levels, self.perm, self.sep_sizes, self.cl_idx, self.cl_interval, self.cl_sep, row, col, val)


def build(tmp_path, name, spec):
    """(tree, separator file, cluster file) of a spec."""
    t = Tree(spec)
    ordf, clustf = t.write(os.path.join(str(tmp_path), name))
    return t, ordf, clustf


def assert_same_plan(a, b):
    """Two plans of the same input (from files, from arrays) are the same plan."""
    assert (a.n, a.levels, a.nsep, a.num_blocks, a.arena_doubles, a.nnz_a, a.dropped) == (b.n, b.levels, b.nsep, b.num_blocks, b.arena_doubles, b.nnz_a, b.dropped)
    assert np.array_equal(a.perm, b.perm) and np.array_equal(a.sep_sizes, b.sep_sizes) and np.array_equal(a.blocks, b.blocks)
    assert np.array_equal(a.fill_host(), b.fill_host())


def cached(tmp_path_factory, name):
    """spd_inputs.cached for every name: the inputs of spd_inputs.INPUTS and the single-purpose trees."""
    import spd_inputs as si
    if name in si.NAMES:
        return si.cached(tmp_path_factory, name)
    spec = TREES[name]
    return si.cached(tmp_path_factory, name, build=lambda tmp_path: si.SPD(tmp_path, spec, 3000 + spec["seed"], name=name))


def sweep(tmp_path, position, s, leaf="dense", oracle=True):
    """The sweep's input for (position, s, leaf): one test each, so not cached."""
    import spd_inputs as si
    spec = sweep_spec(position, s, leaf)
    return si.SPD(str(tmp_path), spec, 3000 + spec["seed"], name=f"sweep_{position}_{s}", oracle=oracle)
