"""Inputs of the macro-tile update tests (a helper module, not a conftest): tests/test_update_mt_host.py, tests/test_gpu_update_mt.py.

The 64 x 64 macro-tile update kernels (k_update_mt, k32_update_mt) are the level schedule's path from mt_min_tiles = 8192 sub-tiles a phase; option
mt_min_tiles = 1 puts every target of more than 16 rows or columns on them.  The cases put the separator of s columns of tree_inputs.sweep_spec

  as the TARGET (middle, root): tiles of 1, 15, 16, 17, 63 and 64 valid rows and columns, one, two and three macro tiles a side, SYRK tiles on and
    off the diagonal;
  as the SOURCE (leaf): K below one 16-deep chunk, exactly one, two and three chunks, and one column over; ("band", 17) leaves, whose sources start
    behind the leaf's first columns (leaf_trim_source);
  under "tiles" couplings: targets next to tiles without storage;

next to the named trees tree_skew, tree_top (random tile boundaries, 1-column separators, a 433-column root), tree_over (pivot failures) and
tree_deep (more than 32 sources a task).  CASES maps a name to (spec, heap index of the separator, its columns)."""
import tree_inputs as ti

TARGET_SIZES = [17, 31, 32, 33, 63, 64, 65, 79, 80, 81, 127, 128, 129, 191, 192, 193]
SOURCE_SIZES = [1, 5, 15, 16, 17, 31, 32, 33, 47, 48, 49]
BAND_SIZES = [193, 259]
HEAP = {"leaf": 4, "middle": 2, "root": 1}

CASES = {}
for _pos in ("middle", "root"):
    for _s in TARGET_SIZES:
        CASES[f"target_{_pos}_{_s}"] = (ti.sweep_spec(_pos, _s), HEAP[_pos], _s)
for _s in SOURCE_SIZES:
    CASES[f"source_leaf_{_s}"] = (ti.sweep_spec("leaf", _s), HEAP["leaf"], _s)
for _s in BAND_SIZES:
    CASES[f"source_band17_{_s}"] = (ti.sweep_spec("leaf", _s, ("band", 17)), HEAP["leaf"], _s)
for _pos, _s in (("leaf", 39), ("middle", 65)):
    CASES[f"tiles_{_pos}_{_s}"] = (dict(ti.sweep_spec(_pos, _s), coupling=["tiles"]), HEAP[_pos], _s)
NAMES = list(CASES)
TREES = ["tree_over", "tree_skew", "tree_top", "tree_deep"]          # the named trees these tests factor whole

MT_PATHS = [{"program": 0, "mt_min_tiles": 1, "merge_targets": 0}, {"program": 0, "mt_min_tiles": 1, "merge_targets": 1}]


def spd(tmp_path, name, oracle=True, dense=True):
    import spd_inputs as si
    spec = CASES[name][0]
    return si.SPD(str(tmp_path), spec, 3000 + spec["seed"], name="mt_" + name, oracle=oracle, dense=dense)


def classes(plan, mt_min_tiles=1, f32=False, rank=0, world=1, dist_top=2, merge=(0, 1)):
    """Plan.level_mt_classes summed over the levels and the merge settings (max_sources: the largest, dma_slack: the least)."""
    tot = {}
    for m in merge:
        for level in range(plan.levels):
            for k, v in plan.level_mt_classes(level, m, mt_min_tiles, f32, rank, world, dist_top).items():
                if k == "max_sources":
                    tot[k] = max(tot.get(k, 0), v)
                elif k == "dma_slack":
                    tot[k] = v if tot.get(k, -1) < 0 else tot[k] if v < 0 else min(tot[k], v)
                else:
                    tot[k] = tot.get(k, 0) + v
    return tot
