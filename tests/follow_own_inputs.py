"""Trees for the tests of the followers' own tiles (a helper module, not a conftest): tests/test_follow_own_host.py, tests/test_gpu_follow_own.py.

A POTRF job of the one-launch factor that follows its sources adds its own tiles to the followed sums at a place the schedule fixes per job
(chol_job.mode, option follow_own): after the last followed column tile where early update jobs write its diagonal block (a "wide" follower,
more than four column tiles, whose sources have more than follow_tail column tiles), in front of the round of its last two items otherwise.
Sizes are in heap order; inner separators and the coupling with the parent are dense (every column tile of a child reaches its parent's diagonal
block), the couplings above the parent are "tiles"."""
import tree_inputs as ti


def _coupling(levels):
    """Coupling kinds in the order tree_inputs cycles them (c = 2, 3, ...; r = parent, grandparent, ...): dense with the parent, "tiles" above."""
    out = []
    for c in range(2, 1 << levels):
        r = c // 2
        while r >= 1:
            out.append("dense" if r == c // 2 else "tiles")
            r //= 2
    return out


def _spec(sizes, seed):
    levels = (len(sizes) + 1).bit_length() - 1
    assert len(sizes) == (1 << levels) - 1
    return dict(levels=levels, sizes=sizes, tile=16, leaf=["dense"], inner=["dense"], coupling=_coupling(levels), seed=seed)


SPECS = {
    # wide followers of 8, 7 and 6 column tiles with ragged last tiles, early tiles from both children; every round is a pair
    "wide_876": _spec([113, 97, 81, 65, 80, 49, 64], 201),
    # the edge of "wide" (5 column tiles against 4); children of exactly 3 column tiles bring no early tile: early jobs from one child only
    "edge_54": _spec([65, 64, 80, 48, 49, 64, 33], 202),
    # followers of 10 and 9 column tiles: single rounds (two column tiles of more than 8 tiles do not share an LDS buffer)
    "single_109": _spec([160, 144, 129, 64, 65, 80, 81], 203),
    # split pivots at the root: the later column blocks follow the strips of the block before them (follow_tail_split)
    "split_177": ti.sweep_spec("root", 177),
    "split_289": ti.sweep_spec("root", 289),
    # four levels: a follower with waits but no early jobs (narrow: the default place) next to wide ones
    "four_levels": _spec([113, 97, 81, 49, 33, 64, 65, 17, 5, 21, 29, 37, 5, 17, 33], 204),
}
NAMES = list(SPECS)
FOLLOW_OWN = [0, 1, 2]


def spd(tmp_path, name, oracle=True):
    import spd_inputs as si
    spec = SPECS[name]
    return si.SPD(str(tmp_path), spec, 3000 + spec["seed"], name="own_" + name, oracle=oracle)
