"""CPU test: the plans of tests/update_mt_cases.py hold the cases the macro-tile update kernels can go wrong on (no device, no oracle).

Plan.level_mt_classes builds a level's lists as the device does and classifies the macro-tile tasks and their sources.  With mt_min_tiles = 1,
summed over the levels and over merge_targets = 0 and 1 (`-s` prints every line):

  input            n     tasks full edge lower mv=1 nv=1  most sources  K<16  16m  16m+1 other  (fp64 schedule; default options: 0 tasks everywhere)
  tree_over       1063    292   52  240   60    18   22        4          94   106   294    0
  tree_skew       1003    561   89  472   60    38   76        7         331   280   407  142
  tree_top         967    938  115  823   80   116   87        4         293   144  1404    0
  tree_deep       1634    429    6  423   26     0    0       64        1160   103   205  712   (7 tasks of 32 sources, 2 of 33 .. 63, 1 of 64;
                                                                                                3 with whole chunks behind the 32nd source)
  target_middle_s  159 .. 335   15 .. 52 tasks; full tiles from s = 64; mv = 1 and nv = 1 at s = 65, 129, 193
  target_root_s    159 .. 335   11 .. 85 tasks; mv = 1 at s = 65, 129, 193; up to 46 sources of K = 16 m + 1
  source_leaf_s    143 .. 191    9 tasks; K < 16 for s = 1, 5, 15, whole chunks at 16, 32, 48, one column over at 17, 33, 49
  source_band17_s  335, 401     13 tasks (fp32: 17 at 259)
  tiles_leaf_39, tiles_middle_65: 8 and 19 tasks, mv = 1 and nv = 1 at middle_65
  (tree_at: 176 tasks, tree_tiny: none -- its targets are at most 16 x 16)

The fp32 schedule cuts pivots wider than 128 columns, so its lists are longer where a separator is wider than that (tree_over 332, tree_skew 577,
tree_top 954, target_middle_129 34, target_root_129 50 tasks) and equal elsewhere.

Every edge tile is served by LDS-DMA: the register-staged fallback of the kernels' bound check never runs (test_no_edge_tile_fails_the_dma_bound
says why no input can reach it)."""
import pytest

import tree_inputs as ti
import update_mt_cases as mc

KEYS = ("tasks", "full", "edge_dma", "edge_staged", "lower", "lower_ar", "mv1", "nv1", "max_sources", "sources_32", "sources_33_63", "sources_64",
        "k_short", "k_chunks", "k_chunks_1", "k_other", "odd_origin", "late_chunks", "empty_ring", "dma_slack")


def test_view_names_follow_the_header():
    """Plan.MT_CLASSES names the counters of cholamd_plan_level_mt_classes in the order of the header's CHOLAMD_MT_* constants."""
    import re
    import cholesky_amd as ca
    from cholesky_amd import _lib
    names = re.findall(r"^  CHOLAMD_MT_([A-Z0-9_]+)", open(_lib.HEADER_PATH).read(), flags=re.M)
    assert names[-1] == "CLASSES" and tuple(n.lower() for n in names[:-1]) == ca.Plan.MT_CLASSES


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """name -> plan of every input of update_mt_cases (the sweep cases without oracle and dense references) and of the named trees."""
    cache = {}

    def get(name):
        if name not in cache:
            cache[name] = (ti.cached(tmp_path_factory, name) if name in ti.TREES else
                           mc.spd(tmp_path_factory.mktemp("mt"), name, oracle=False, dense=False)).plan
        return cache[name]
    return get


def _line(name, P, f32, c):
    return f"{name:18s} n {P.n:5d} {'fp32' if f32 else 'fp64'} " + " ".join(f"{k}={c[k]}" for k in KEYS)


def _all(plans, f32):
    out = {}
    for name in mc.TREES + mc.NAMES:
        out[name] = mc.classes(plans(name), 1, f32)
        print(_line(name, plans(name), f32, out[name]))
    return out


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_every_input_reaches_the_macro_tiles_only_when_forced(f32, plans):
    """mt_min_tiles = 1: macro-tile tasks on every named tree and every sweep case; at the default threshold: none, on any level, merged or not --
    the suite's trees never ran these kernels before."""
    for name in mc.TREES + mc.NAMES:
        forced, default = mc.classes(plans(name), 1, f32), mc.classes(plans(name), -1, f32)
        print(_line(name, plans(name), f32, forced))
        assert forced["tasks"] > 0 and default["tasks"] == 0, name
    for name in ("tree_at", "tree_tiny"):
        print(_line(name, plans(name), f32, mc.classes(plans(name), 1, f32)))


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_tree_deep_fills_more_than_one_descriptor_batch(f32, plans):
    """Tasks of exactly 32 sources (src_end - sb == 32 ends the batch loop), of 33 .. 63 (a full batch and a partial one) and of 64 or more
    (two full ones); behind the 32nd source of a task there are sources of k >= 16, so the ring issues chunks after its restart."""
    c = mc.classes(plans("tree_deep"), 1, f32)
    print(_line("tree_deep", plans("tree_deep"), f32, c))
    assert c["sources_32"] > 0 and c["sources_33_63"] > 0 and c["sources_64"] > 0 and c["max_sources"] >= 64
    assert c["late_chunks"] > 0
    for name in mc.TREES[:-1] + mc.NAMES:                # nothing else gets there
        assert mc.classes(plans(name), 1, f32)["max_sources"] < 32, name


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_the_inputs_hold_every_class(f32, plans):
    """Across the inputs: tiles of one valid row and of one valid column, full tiles, `lower` tiles on and below the first diagonal tile, sources of
    every K class (shorter than a chunk, whole chunks, one column over, other), DMA-served tiles whose ring stays empty, odd operand origins."""
    tot = {}
    for c in _all(plans, f32).values():
        for k in KEYS:
            tot[k] = tot.get(k, 0) + c[k]
    for k in ("mv1", "nv1", "full", "edge_dma", "lower", "lower_ar", "k_short", "k_chunks", "k_chunks_1", "k_other", "empty_ring", "odd_origin"):
        assert tot[k] > 0, k
    # the sweep alone (each case its own GPU test): the same without the named trees
    sweep = {k: sum(mc.classes(plans(n), 1, f32)[k] for n in mc.NAMES) for k in KEYS}
    for k in ("mv1", "nv1", "full", "lower", "lower_ar", "k_short", "k_chunks", "k_chunks_1", "k_other", "empty_ring"):
        assert sweep[k] > 0, k


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_no_edge_tile_fails_the_dma_bound(f32, plans):
    """The kernels serve an edge tile by LDS-DMA when 64 rows of every source's whole chunks lie inside the arena, else they stage it through
    registers.  The failing side has no input: the DMA of a tile reaches at most 63 elements beyond the source panel's last element, and a
    macro-tile target has more than 16 rows or columns, which are columns of an ANCESTOR of the source -- a separator of at least 17 columns whose
    own panel (17 x 17 elements or more) lies behind the source's panel in the arena (panels are stored in elimination order, the root last).  This
    rests on a target's rows all coming from ONE separator, as they do: targets are merged inside one block only.  So at
    least 17 * 17 - 63 = 226 elements remain between the furthest DMA element and the arena's end on every input; a root of one column does not
    change it (its own tiles are 16 x 16 tasks, not macro tiles).  The fallback runs only for a caller without the arena's length (arena_elems = 0),
    which the library never is; this test holds the statement on every input, ranks of a distributed top included."""
    for name in mc.TREES + mc.NAMES:
        c = mc.classes(plans(name), 1, f32)
        assert c["edge_dma"] > 0 and c["edge_staged"] == 0 and c["dma_slack"] >= 226, (name, c)
    for world in (2, 4):
        for rank in range(world):
            c = mc.classes(plans("tree_top"), 1, f32, rank, world, 1)
            assert c["edge_staged"] == 0 and c["dma_slack"] >= 226, (world, rank, c)


@pytest.mark.parametrize("f32", [False, True], ids=["fp64", "fp32"])
def test_distributed_top_cuts_syrk_targets_at_column_blocks(f32, plans):
    """tree_top under a distributed top (dist_top = 1): every rank of worlds 2 and 4 has macro-tile tasks under mt_min_tiles = 1 and none at the
    default, `lower` tiles with ar != 0 among them, and in each world some whose origin is no multiple of 64: push_tasks cuts a SYRK target at the
    separator's column blocks (112 columns), the only place where a target's own origin (ar0, br0) is not zero."""
    P = plans("tree_top")
    for world in (2, 4):
        cut = 0
        for rank in range(world):
            c = mc.classes(P, 1, f32, rank, world, 1)
            print(_line(f"tree_top {rank}/{world}", P, f32, c) + f" lower_ar_cut={c['lower_ar_cut']}")
            assert c["tasks"] > 0 and mc.classes(P, -1, f32, rank, world, 1)["tasks"] == 0, (world, rank)
            assert c["lower_ar"] > 0, (world, rank)
            cut += c["lower_ar_cut"]
        assert cut > 0, world                              # (world 2: rank 1's, world 4: ranks 0 and 3)
    assert mc.classes(P, 1, f32)["lower_ar_cut"] == 0      # one GPU: origins are multiples of 64
