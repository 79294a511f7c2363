"""Host-side plan: ingest + symbolic analysis (the part of mmat.rg's main before the level loop,
mmat.rg:1097-1209), computed by the C library."""
import ctypes as C
import os

import numpy as np

from ._lib import Filled, Op, check, load

OP_NAMES = ("POTRF", "TRSM", "SYRK", "GEMM")


class Plan:
    def __init__(self, matrix_file=None, separator_file=None, clusters_file=None, _handle=None):
        self.L = load()
        if _handle is not None:
            self.h = _handle
        else:
            h = C.c_void_p()
            check(self.L.cholamd_plan_create(os.fsencode(matrix_file), os.fsencode(separator_file), os.fsencode(clusters_file), C.byref(h)),
                  "cholamd_plan_create")
            self.h = h
        g = self.L
        self.n = g.cholamd_plan_n(self.h)
        self.nz = g.cholamd_plan_nz(self.h)
        self.levels = g.cholamd_plan_levels(self.h)
        self.nsep = g.cholamd_plan_num_separators(self.h)
        self.num_blocks = g.cholamd_plan_num_blocks(self.h)
        self.arena_doubles = g.cholamd_plan_arena_doubles(self.h)
        self.flops = g.cholamd_plan_flops(self.h)          # F_ref
        self.alg_bytes = g.cholamd_plan_alg_bytes(self.h)  # B_alg
        self.nnz_a = g.cholamd_plan_nnz_a(self.h)
        self.nnz_l = g.cholamd_plan_nnz_l(self.h)
        self.nnz_tiles = g.cholamd_plan_nnz_tiles(self.h)
        self.fmin = g.cholamd_plan_fmin(self.h)
        self.dropped = g.cholamd_plan_dropped_entries(self.h)
        self.max_int_size = g.cholamd_plan_max_int_size(self.h)

    @classmethod
    def from_arrays(cls, n, levels, perm, sep_sizes, cl_idx, cl_interval, cl_sep, a_row, a_col, a_val, banner=None):
        L = load()
        arr = lambda a, t: np.ascontiguousarray(a, dtype=t)  # noqa: E731
        perm, sep_sizes = arr(perm, np.int32), arr(sep_sizes, np.int32)
        cl_idx, cl_interval, cl_sep = arr(cl_idx, np.int32), arr(cl_interval, np.int32), arr(cl_sep, np.int32)
        a_row, a_col, a_val = arr(a_row, np.int32), arr(a_col, np.int32), arr(a_val, np.float64)
        h = C.c_void_p()
        check(L.cholamd_plan_create_from_arrays(n, levels, perm.ctypes.data, sep_sizes.ctypes.data, cl_idx.ctypes.data,
                                                cl_interval.ctypes.data, cl_sep.ctypes.data, len(cl_idx), len(a_val),
                                                a_row.ctypes.data, a_col.ctypes.data, a_val.ctypes.data,
                                                banner.encode() if banner else None, C.byref(h)), "cholamd_plan_create_from_arrays")
        return cls(_handle=h)

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.cholamd_plan_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def _ints(self, fn, n):
        a = np.zeros(n, dtype=np.int32)
        getattr(self.L, fn)(self.h, a.ctypes.data)
        return a

    @property
    def banner(self):
        return self.L.cholamd_plan_banner(self.h).decode()

    @property
    def perm(self):
        return self._ints("cholamd_plan_perm", self.n)

    @property
    def sep_sizes(self):
        return self._ints("cholamd_plan_sep_sizes", self.nsep)

    @property
    def sep_offsets(self):
        return self._ints("cholamd_plan_sep_offsets", self.nsep)

    @property
    def tree(self):
        return self._ints("cholamd_plan_tree", self.nsep)

    @property
    def blocks(self):
        """rows: r, c, lo_x, lo_y, hi_x, hi_y, ld, arena offset (int64)"""
        raw = self._ints("cholamd_plan_blocks", 9 * self.num_blocks).reshape(-1, 9).astype(np.int64)
        off = (raw[:, 7] & 0xFFFFFFFF) | (raw[:, 8] << 32)
        return np.concatenate([raw[:, :7], off[:, None]], axis=1)

    def heap_of(self, label):
        """Heap index (root = 1, children of h = 2 h, 2 h + 1) of a separator label."""
        return int(np.nonzero(self.tree == label)[0][0]) + 1

    @property
    def arena_dense_doubles(self):
        """What the arena would hold with every ancestor row stored (no row compaction)."""
        return int(self.L.cholamd_plan_arena_dense_doubles(self.h))

    def block_tile_map(self, r, c):
        """Stored position of every 16-row tile of block (r, c) in its panel (-1: the tile has no storage)."""
        rows = int(self.sep_sizes[r - 1])
        out = np.zeros((rows + 15) // 16 + 1, dtype=np.int32)
        n = self.L.cholamd_plan_block_tile_map(self.h, r, c, out.ctypes.data)
        if n < 0:
            raise ValueError(f"no block ({r}, {c})")
        return out[:n]

    def snapshot(self, interval_lbl):
        n = self.L.cholamd_plan_snapshot_count(self.h, interval_lbl)
        buf = (Filled * max(n, 1))()
        self.L.cholamd_plan_snapshot(self.h, interval_lbl, buf)
        return buf, n

    def snapshot_array(self, interval_lbl):
        buf, n = self.snapshot(interval_lbl)
        a = np.frombuffer(buf, dtype=np.int32).reshape(-1, 9)[:n]
        return a[:, [1, 2, 4, 5, 6, 7, 8]].copy()  # sep_x, sep_y, cluster, lo_x, lo_y, hi_x, hi_y

    def ops(self):
        n = self.L.cholamd_plan_num_ops(self.h)
        buf = (Op * max(n, 1))()
        self.L.cholamd_plan_ops(self.h, buf)
        return np.frombuffer(buf, dtype=np.int32).reshape(-1, 14)[:n].copy()

    def counts(self, level=-1):
        c = np.zeros(4, dtype=np.int64)
        f = np.zeros(4, dtype=np.float64)
        self.L.cholamd_plan_counts(self.h, level, c.ctypes.data, f.ctypes.data)
        return c, f

    def entries(self):
        """(row, col) of the entry list in value-array order: original 0-based coordinates, in the order plan creation received them
        (cholamd_plan_entries).  Entry k of a value array (fill_host(values), Device.set_values) is the value of entry k of this list."""
        row, col = np.zeros(self.nz, dtype=np.int32), np.zeros(self.nz, dtype=np.int32)
        check(self.L.cholamd_plan_entries(self.h, row.ctypes.data, col.ctypes.data), "cholamd_plan_entries")
        return row, col

    def value_map(self):
        """Index in the value array of every scatter entry (nnz_a of them, ascending arena offset): cholamd_plan_value_map.  The indices that
        do not occur are outside the pattern (0.0 at creation) or were dropped by the ordering."""
        out = np.zeros(self.nnz_a, dtype=np.int64)
        check(self.L.cholamd_plan_value_map(self.h, out.ctypes.data), "cholamd_plan_value_map")
        return out

    def fill_host(self, values=None):
        """fill_block for every block: the arena holding P A P^T (host array).  `values`: a value array of `nz` doubles (see entries()) to
        scatter instead of the plan's own values."""
        a = np.zeros(self.arena_doubles, dtype=np.float64)
        if values is None:
            check(self.L.cholamd_plan_fill_host(self.h, a.ctypes.data), "cholamd_plan_fill_host")
        else:
            v = np.ascontiguousarray(values, dtype=np.float64)
            check(self.L.cholamd_plan_fill_host_values(self.h, v.ctypes.data, v.size, a.ctypes.data), "cholamd_plan_fill_host_values")
        return a

    @property
    def duplicate_entries(self):
        """In-pattern entries that repeat the position of another one (cholamd_plan_duplicate_entries): the values-gradient calls refuse such a plan."""
        return int(self.L.cholamd_plan_duplicate_entries(self.h))

    def values_grad_pairs_host(self, P, Q, alpha=1.0, beta=0.0, g=None, ldp=None, ldq=None):
        """Device.values_grad_pairs on the CPU (cholamd_plan_values_grad_pairs_host): the same walk with fma(), the device's bits.  P, Q: n x nrhs
        arrays (Q may be P itself: then one buffer is handed over twice); g: plan.nz doubles to accumulate into (a copy is returned), NaN-filled when
        None.  ldp / ldq: leading dimensions of the column-major copies handed to the library (default n); the rows behind are -3.0 and never read."""
        P = np.asarray(P, dtype=np.float64)
        assert P.ndim == 2 and P.shape[0] == self.n
        k = P.shape[1]
        ldp, ldq = int(ldp or self.n), int(ldq or self.n)
        pb = self._colmajor(P, self.n, ldp, -3.0)
        if Q is P:
            assert ldq == ldp
            qb = pb
        else:
            Q = np.asarray(Q, dtype=np.float64)
            assert Q.shape == P.shape
            qb = self._colmajor(Q, self.n, ldq, -3.0)
        out = np.full(max(self.nz, 1), np.nan) if g is None else np.array(g, dtype=np.float64)
        check(self.L.cholamd_plan_values_grad_pairs_host(self.h, pb.ctypes.data, ldp, qb.ctypes.data, ldq, k, float(alpha), float(beta), out.ctypes.data, self.nz),
              "cholamd_plan_values_grad_pairs_host")
        return out[:self.nz]

    def values_grad_logdet_host(self, zarena, alpha=1.0, beta=0.0, g=None):
        """Device.values_grad_logdet on the CPU from a host copy of the Z arena (cholamd_plan_values_grad_logdet_host); g as for values_grad_pairs_host."""
        zarena = np.ascontiguousarray(zarena, dtype=np.float64)
        assert zarena.size == self.arena_doubles
        out = np.full(max(self.nz, 1), np.nan) if g is None else np.array(g, dtype=np.float64)
        check(self.L.cholamd_plan_values_grad_logdet_host(self.h, zarena.ctypes.data, float(alpha), float(beta), out.ctypes.data, self.nz),
              "cholamd_plan_values_grad_logdet_host")
        return out[:self.nz]

    def fill_host_part(self, rank, world):
        """Host arena as rank `rank` of `world` starts from (A's shared-top entries on rank 0 only) and
        the offset of the shared tail of the arena."""
        a = np.zeros(self.arena_doubles, dtype=np.float64)
        tail = C.c_int64(0)
        check(self.L.cholamd_plan_fill_host_part(self.h, a.ctypes.data, rank, world, C.byref(tail)), "cholamd_plan_fill_host_part")
        return a, tail.value

    def level_work_counts(self, level, rank=0, world=1):
        out = np.zeros(4, dtype=np.int32)
        check(self.L.cholamd_plan_level_work_counts(self.h, level, rank, world, out.ctypes.data), "cholamd_plan_level_work_counts")
        return tuple(int(v) for v in out)

    def exchange_volume(self, rank, world, dist_top=2):
        """(received, sent, tail, pieces) in arena elements of the extend-add exchange of (rank, world): cholamd_plan_exchange_volume."""
        out = np.zeros(4, dtype=np.int64)
        check(self.L.cholamd_plan_exchange_volume(self.h, rank, world, dist_top, out.ctypes.data), "cholamd_plan_exchange_volume")
        return tuple(int(v) for v in out)

    def solve_counts(self, level, rank=0, world=1):
        """(separators, row runs, forward chunks, backward chunks, columns solved) of one rank's solve lists of a level (cholamd_plan_solve_counts)."""
        out = np.zeros(5, dtype=np.int64)
        check(self.L.cholamd_plan_solve_counts(self.h, level, rank, world, out.ctypes.data), "cholamd_plan_solve_counts")
        return tuple(int(v) for v in out)

    def solve_skips(self, level):
        """(seps, runs) of cholamd_plan_solve_skips: rows (first position, columns, band) per separator and (first row position, rows, first column
        position, columns, c_lo) per (ancestor, separator) row run of the level's solve lists."""
        cnt = self.solve_counts(level)
        seps = np.zeros((max(cnt[0], 1), 3), dtype=np.int32)
        runs = np.zeros((max(cnt[1], 1), 5), dtype=np.int32)
        check(self.L.cholamd_plan_solve_skips(self.h, level, seps.ctypes.data, runs.ctypes.data), "cholamd_plan_solve_skips")
        return seps[:cnt[0]], runs[:cnt[1]]

    def diag_list(self):
        """cholamd_plan_diag_list: where the factor's diagonal lies in an arena -- (a_off int64, cols, lda, x_off, sep, prefix) with one entry per
        separator in the order of the permuted vector (prefix: one more); element j of descriptor i is arena[a_off[i] + j * (lda[i] + 1)]."""
        m = self.nsep
        a_off = np.zeros(m, dtype=np.int64)
        cols, lda, x_off, sep = (np.zeros(m, dtype=np.int32) for _ in range(4))
        prefix = np.zeros(m + 1, dtype=np.int32)
        n = self.L.cholamd_plan_diag_list(self.h, a_off.ctypes.data, cols.ctypes.data, lda.ctypes.data, x_off.ctypes.data, sep.ctypes.data, prefix.ctypes.data)
        if n < 0:
            check(n, "cholamd_plan_diag_list")
        return a_off[:n], cols[:n], lda[:n], x_off[:n], sep[:n], prefix[:n + 1]

    SELINV_BLOCK = 64         # CHOLAMD_SELINV_BLOCK: columns of a column block of the selected inversion
    SELINV_FRONT_MAX = 8192   # CHOLAMD_SELINV_FRONT_MAX: most rows below a block selinv_front tabulates

    def selinv_blocks(self, sep):
        """Column blocks of separator `sep` (label) in the selected inversion (cholamd_plan_selinv_blocks)."""
        n = self.L.cholamd_plan_selinv_blocks(self.h, int(sep))
        if n < 0:
            check(n, "cholamd_plan_selinv_blocks")
        return n

    def selinv_front(self, sep, block):
        """Host view of the gather lists of Device.selinv for column block `block` of separator `sep` (cholamd_plan_selinv_front):
        (first column's permuted position, columns, pos, off) -- pos[i] = permuted positions of the m rows below the block, off[i, j] = Z-arena offset
        of Z(pos[i], pos[j]) (the stored side) or -1 = not stored, read as 0.0.  Quadratic in m; refuses m > SELINV_FRONT_MAX."""
        cols = np.zeros(2, dtype=np.int32)
        m = self.L.cholamd_plan_selinv_front(self.h, int(sep), int(block), 0, cols.ctypes.data, None, None)
        if m < 0:
            check(m, "cholamd_plan_selinv_front")
        pos = np.zeros(max(m, 1), dtype=np.int32)
        off = np.zeros((max(m, 1), max(m, 1)), dtype=np.int64)
        m2 = self.L.cholamd_plan_selinv_front(self.h, int(sep), int(block), m, cols.ctypes.data, pos.ctypes.data, off.ctypes.data)
        if m2 < 0:
            check(m2, "cholamd_plan_selinv_front")
        return int(cols[0]), int(cols[1]), pos[:m], off[:m, :m]

    def exchange_pieces(self, world, dist_top=2):
        """The column-block pieces of that exchange as rows (arena offset, elements, owner rank, heap index of the top separator)."""
        out = np.zeros((4096, 4), dtype=np.int64)
        n = self.L.cholamd_plan_exchange_pieces(self.h, world, dist_top, len(out), out.ctypes.data)
        if n < 0:
            check(n, "cholamd_plan_exchange_pieces")
        return out[:min(n, len(out))]

    def level_work_volume(self, level, rank=0, world=1, dist_top=2):
        """(POTRF columns, TRSM elements, update volume, broadcast entries, broadcast doubles, broadcast checksum) of one level's
        lists for (rank, world) with the top levels replicated (dist_top=0), distributed by column blocks (1) or automatic (2)."""
        out = np.zeros(6, dtype=np.int64)
        check(self.L.cholamd_plan_level_work_volume(self.h, level, rank, world, dist_top, out.ctypes.data), "cholamd_plan_level_work_volume")
        return tuple(int(v) for v in out)

    def level_work_volume_opts(self, level, merge_targets=1, mt_min_tiles=-1):
        """level_work_volume (single GPU) under option merge_targets / mt_min_tiles + (16x16 tasks, macro-tile tasks, TRSM strips)."""
        out = np.zeros(9, dtype=np.int64)
        check(self.L.cholamd_plan_level_work_volume_opts(self.h, level, int(merge_targets), int(mt_min_tiles), out.ctypes.data), "cholamd_plan_level_work_volume_opts")
        return tuple(int(v) for v in out)

    def level_mt_fill(self, level):
        """(macro-tile tasks, tasks with all 64 x 64 elements valid, valid elements x depth, tile elements x depth) of one level's lists."""
        out = np.zeros(4, dtype=np.int64)
        check(self.L.cholamd_plan_level_mt_fill(self.h, level, out.ctypes.data), "cholamd_plan_level_mt_fill")
        return tuple(int(v) for v in out)

    MT_CLASSES = ("tasks", "full", "edge_dma", "edge_staged", "lower", "lower_ar", "mv1", "nv1", "max_sources", "sources_32", "sources_33_63",
                  "sources_64", "k_short", "k_chunks", "k_chunks_1", "k_other", "odd_origin", "late_chunks", "lower_ar_cut", "empty_ring", "dma_slack")

    def level_mt_classes(self, level, merge_targets=1, mt_min_tiles=-1, f32=False, rank=0, world=1, dist_top=2):
        """What the macro-tile update kernels meet on one level's lists (cholamd_plan_level_mt_classes): a dict of counts by MT_CLASSES -- tasks,
        full 64 x 64 tiles, edge tiles served by LDS-DMA / staged through registers, `lower` tiles (and those with ar != 0), tiles of one valid
        row / column, the most sources of a task and the tasks with 32, 33 .. 63 and >= 64, sources by depth (k < 16, whole chunks, one column
        over, other), sources of odd operand origin, tasks whose ring issues chunks in a second descriptor batch, `lower` tiles with ar % 64 != 0 (cut at a column block),
        DMA-served tiles with no whole chunk, the least distance between an edge tile's furthest DMA element and the arena's end (-1: none)."""
        out = np.zeros(len(self.MT_CLASSES), dtype=np.int64)
        check(self.L.cholamd_plan_level_mt_classes(self.h, level, int(merge_targets), int(mt_min_tiles), int(bool(f32)), rank, world, dist_top,
                                                   out.ctypes.data), "cholamd_plan_level_mt_classes")
        return dict(zip(self.MT_CLASSES, (int(v) for v in out)))

    def program_check(self, follow=True, workers=64):
        """Host-side self-check of the one-launch program (raises CholamdError on a dead-lock or a mismatch)."""
        check(self.L.cholamd_plan_program_check(self.h, int(follow), int(workers)), "cholamd_plan_program_check")

    def program_check_opts(self, follow_tail=-1, split_min=-1, split_nb=-1, workers=64, follow_tail_split=-1, follow_own=-1):
        """program_check under other follower tails / pivot splits / places of the followers' own tiles (negative: the default)."""
        check(self.L.cholamd_plan_program_check_follow(self.h, follow_tail, follow_tail_split, follow_own, split_min, split_nb, int(workers)),
              "cholamd_plan_program_check_follow")

    def program_follow_own(self, follow_own=-1, follow_tail=-1, follow_tail_split=-1, split_min=-1, split_nb=-1):
        """The following POTRF jobs of the one-launch program under the given options (negative: the default), one dict each: job, n_ext (followed
        column tiles), T (column tiles of the block), own_at (the item in front of whose round the job adds its own tiles; n_ext: after the last
        item -- the place the kernel takes from the job), n_wait (0: the job loads its own tiles first)."""
        n = self.L.cholamd_plan_program_follow_own(self.h, follow_tail, follow_tail_split, follow_own, split_min, split_nb, 0, None)
        if n < 0:
            check(int(n), "cholamd_plan_program_follow_own")
        buf = np.zeros(5 * n + 5, dtype=np.int32)
        self.L.cholamd_plan_program_follow_own(self.h, follow_tail, follow_tail_split, follow_own, split_min, split_nb, buf.size, buf.ctypes.data)
        return [dict(zip(("job", "n_ext", "T", "own_at", "n_wait"), (int(v) for v in buf[5 * i:5 * i + 5]))) for i in range(n)]

    def program_hazards(self, follow_own=-1, follow_tail=-1, follow_tail_split=-1, split_min=-1, split_nb=-1):
        """Write hazards between the update jobs of the one-launch program: (pairs of update jobs that write a common arena element, pairs among them
        whose later job may start before the earlier one has completed, the first such pair or (-1, -1))."""
        out = np.zeros(4, dtype=np.int32)
        check(self.L.cholamd_plan_program_hazards(self.h, follow_tail, follow_tail_split, follow_own, split_min, split_nb, out.ctypes.data), "cholamd_plan_program_hazards")
        return int(out[0]), int(out[1]), (int(out[2]), int(out[3]))

    def program_counts(self, follow=True):
        out = np.zeros(6, dtype=np.int32)
        check(self.L.cholamd_plan_program_counts(self.h, int(follow), out.ctypes.data), "cholamd_plan_program_counts")
        return dict(zip(("jobs", "followers", "tasks", "strips", "counters", "followed_panels"), (int(v) for v in out)))

    def program_jobs(self, follow=True):
        """Diagnostic: (jobs [n, 8] = kind, sep, aux, first, n, sig0, sig1, n_wait; waits [m, 3] = job, counter, value)."""
        need = self.L.cholamd_plan_program_jobs(self.h, int(follow), 0, None)
        buf = np.zeros(need, dtype=np.int32)
        self.L.cholamd_plan_program_jobs(self.h, int(follow), need, buf.ctypes.data)
        nj = int(buf[-1])
        return buf[:8 * nj].reshape(nj, 8), buf[8 * nj:-1].reshape(-1, 3)

    # -- Schur complement on the top k levels of the tree (the host side of Device.schur*) -----------------------------------------
    SCHUR_RECORD = 7  # CHOLAMD_SCHUR_RECORD: int64 words per record of schur_list

    def schur_size(self, k):
        """m = the dofs of the k kept tree levels (heap indices 1 .. 2^k - 1): cholamd_plan_schur_size.  They are permuted positions [n - m, n)."""
        m = self.L.cholamd_plan_schur_size(self.h, int(k))
        if m < 0:
            check(m, "cholamd_plan_schur_size")
        return m

    def schur_dofs(self, k):
        """The m original dof ids in Schur order (entry i = perm[n - m + i]): cholamd_plan_schur_dofs."""
        m = self.schur_size(k)
        out = np.zeros(max(m, 1), dtype=np.int32)
        check(min(self.L.cholamd_plan_schur_dofs(self.h, int(k), out.ctypes.data), 0), "cholamd_plan_schur_dofs")
        return out[:m]

    def schur_list(self, k):
        """Host view of the gather of Device.schur (cholamd_plan_schur_list): int64 rows (arena offset, leading dimension, rows, columns, first row,
        first column in Schur coordinates, 1 = in a diagonal block: lower triangle only), one per stored 16-row tile piece of a kept block."""
        cnt = self.L.cholamd_plan_schur_list(self.h, int(k), 0, None)
        if cnt < 0:
            check(cnt, "cholamd_plan_schur_list")
        out = np.zeros((max(cnt, 1), self.SCHUR_RECORD), dtype=np.int64)
        check(min(self.L.cholamd_plan_schur_list(self.h, int(k), cnt, out.ctypes.data), 0), "cholamd_plan_schur_list")
        return out[:cnt]

    def schur_host(self, k, arena, lds=None):
        """S (m x m, both triangles) gathered on the CPU from a host arena (cholamd_plan_schur_host): what Device.schur writes, bit for bit.  `lds`:
        leading dimension of the column-major result (default m); the rows m .. lds - 1 are returned as NaN, untouched."""
        arena = np.ascontiguousarray(arena, dtype=np.float64)
        assert arena.size == self.arena_doubles
        m = self.schur_size(k)
        ld = m if lds is None else int(lds)
        buf = np.full((max(m, 1), max(ld, 1)), np.nan, dtype=np.float64)  # row j of the buffer = column j of S
        check(self.L.cholamd_plan_schur_host(self.h, int(k), arena.ctypes.data, buf.ctypes.data, ld), "cholamd_plan_schur_host")
        return buf[:m, :].T if lds is not None else buf[:m, :m].T

    @staticmethod
    def _colmajor(M, rows, ld, fill):
        """A (columns, ld) buffer whose row j holds column j of M (rows x k) and `fill` behind it: the column-major copy handed to the library."""
        k = M.shape[1]
        buf = np.full((max(k, 1), max(ld, 1)), fill, dtype=np.float64)
        buf[:k, :rows] = M.T
        return buf

    def schur_condense_host_nrhs(self, k, arena, B, ldb=None, ldw=None, ldg=None):
        """(W, G) = the block condense on the CPU over a host arena whose levels under the cut are factored (cholamd_plan_schur_condense_host_nrhs): the
        cut step lists of Device option schur_deterministic with the block gather's partition.  B: n x nrhs in original dof order; W: n x nrhs (column
        j = the state w of column j), G: m x nrhs in Schur order.  ld*: leading dimensions of the column-major copies handed to the library (defaults:
        the row counts); the rows behind the arrays are checked to be untouched.  Deterministic, columns independent; not the device's bits."""
        arena = np.ascontiguousarray(arena, dtype=np.float64)
        assert arena.size == self.arena_doubles
        B = np.asarray(B, dtype=np.float64)
        assert B.ndim == 2 and B.shape[0] == self.n
        n, m, c = self.n, self.schur_size(k), B.shape[1]
        ldb, ldw, ldg = int(ldb or n), int(ldw or n), int(ldg or m)
        bb = self._colmajor(B, n, ldb, -3.0)
        wb, gb = np.full((max(c, 1), max(ldw, 1)), np.nan), np.full((max(c, 1), max(ldg, 1)), np.nan)
        check(self.L.cholamd_plan_schur_condense_host_nrhs(self.h, int(k), arena.ctypes.data, bb.ctypes.data, ldb, wb.ctypes.data, ldw, gb.ctypes.data, ldg, c),
              "cholamd_plan_schur_condense_host_nrhs")
        assert np.isnan(wb[:, n:]).all() and np.isnan(gb[:, m:]).all(), "rows behind W or G were written"
        return wb[:c, :n].T.copy(), gb[:c, :m].T.copy()

    def schur_expand_host_nrhs(self, k, arena, W, XT, ldw=None, ldxt=None, ldx=None):
        """X (n x nrhs, original dof order) = the block expand on the CPU from W of schur_condense_host_nrhs and the caller's XT (m x nrhs, Schur order):
        cholamd_plan_schur_expand_host_nrhs.  W is not modified (checked)."""
        arena = np.ascontiguousarray(arena, dtype=np.float64)
        assert arena.size == self.arena_doubles
        W, XT = np.asarray(W, dtype=np.float64), np.asarray(XT, dtype=np.float64)
        n, m = self.n, self.schur_size(k)
        assert W.ndim == 2 and W.shape[0] == n and XT.ndim == 2 and XT.shape == (m, W.shape[1])
        c = W.shape[1]
        ldw, ldxt, ldx = int(ldw or n), int(ldxt or m), int(ldx or n)
        wb, tb = self._colmajor(W, n, ldw, -3.0), self._colmajor(XT, m, ldxt, -3.0)
        w0 = wb.copy()
        xb = np.full((max(c, 1), max(ldx, 1)), np.nan)
        check(self.L.cholamd_plan_schur_expand_host_nrhs(self.h, int(k), arena.ctypes.data, wb.ctypes.data, ldw, tb.ctypes.data, ldxt, xb.ctypes.data, ldx, c),
              "cholamd_plan_schur_expand_host_nrhs")
        assert np.isnan(xb[:, n:]).all(), "rows n .. ldx - 1 of X were written"
        assert wb.tobytes() == w0.tobytes(), "the expand wrote W"
        return xb[:c, :n].T.copy()

    def schur_det_counts(self, k):
        """Sizes of the step lists of condense (forward) and expand (backward) cut at k kept levels (cholamd_plan_schur_det_counts): steps, items,
        sources and the entries of L one sweep reads."""
        out = np.zeros(8, dtype=np.int64)
        check(self.L.cholamd_plan_schur_det_counts(self.h, int(k), out.ctypes.data), "cholamd_plan_schur_det_counts")
        return {w: dict(steps=int(out[4 * i]), items=int(out[4 * i + 1]), sources=int(out[4 * i + 2]), entries=int(out[4 * i + 3]))
                for i, w in enumerate(("forward", "backward"))}

    def schur_det_lists(self, k, which):
        """The cut lists of one direction (cholamd_plan_schur_det_lists) in the formats of solve_det_lists; the kept lead step of the forward list has
        level = -1 (and no span: first column -1)."""
        c = self.schur_det_counts(k)["forward" if which == 0 else "backward"]
        steps = np.zeros((max(c["steps"], 1), 4), dtype=np.int64)
        items = np.zeros((max(c["items"], 1), 4), dtype=np.int64)
        srcs = np.zeros((max(c["sources"], 1), 5), dtype=np.int64)
        check(self.L.cholamd_plan_schur_det_lists(self.h, int(k), int(which), steps.ctypes.data, items.ctypes.data, srcs.ctypes.data), "cholamd_plan_schur_det_lists")
        return steps[:c["steps"]], items[:c["items"]], srcs[:c["sources"]]

    def apply_host(self, x, values=None):
        """y = A x on the CPU in the device's fma order (cholamd_plan_apply_host): bit for bit what Device.apply returns.  values: a value array of
        plan.nz doubles as Device.set_values takes it (None: the plan's own values)."""
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.shape == (self.n,)
        if values is not None:
            values = np.ascontiguousarray(values, dtype=np.float64)
            if values.shape != (self.nz,):
                raise ValueError(f"values must hold plan.nz = {self.nz} doubles; got {values.shape}")
        y = np.full(max(self.n, 1), np.nan, dtype=np.float64)
        check(self.L.cholamd_plan_apply_host(self.h, values.ctypes.data if values is not None else None, x.ctypes.data, y.ctypes.data), "cholamd_plan_apply_host")
        return y[:self.n]

    def multiply_host(self, arena, which, z):
        """y = M z (which = 0) or y = M^T z (1) on the CPU from a host arena (cholamd_plan_multiply_host): the owner lists of Device.multiply_half
        walked on the host -- the lower triangles and the stored row runs only.  z and the result: n doubles in original dof order."""
        arena = np.ascontiguousarray(arena, dtype=np.float64)
        assert arena.size == self.arena_doubles
        z = np.ascontiguousarray(z, dtype=np.float64)
        assert z.shape == (self.n,)
        y = np.full(max(self.n, 1), np.nan, dtype=np.float64)
        check(self.L.cholamd_plan_multiply_host(self.h, arena.ctypes.data, int(which), z.ctypes.data, y.ctypes.data), "cholamd_plan_multiply_host")
        return y[:self.n]

    def multiply_host_nrhs(self, arena, which, Z, ldz=None, ldy=None):
        """Y = M Z (which = 0), M^T Z (1) or M M^T Z (-1) on the CPU for the columns of Z (n x k) with the block kernel's partition of every source
        (cholamd_plan_multiply_host_nrhs).  ldz / ldy: leading dimensions of the column-major copies handed to the library (default n); the rows
        n .. ldy - 1 of the result are checked to be untouched.  Returns n x k."""
        arena = np.ascontiguousarray(arena, dtype=np.float64)
        assert arena.size == self.arena_doubles
        Z = np.asarray(Z, dtype=np.float64)
        assert Z.ndim == 2 and Z.shape[0] == self.n
        k = Z.shape[1]
        ldz, ldy = int(ldz or self.n), int(ldy or self.n)
        zb = np.full((max(k, 1), max(ldz, 1)), -3.0)     # row j of the buffer = column j of Z
        zb[:k, :self.n] = Z.T
        yb = np.full((max(k, 1), max(ldy, 1)), np.nan)
        check(self.L.cholamd_plan_multiply_host_nrhs(self.h, arena.ctypes.data, int(which), zb.ctypes.data, ldz, yb.ctypes.data, ldy, k), "cholamd_plan_multiply_host_nrhs")
        assert np.isnan(yb[:, self.n:]).all(), "rows n .. ldy - 1 of Y were written"
        return yb[:k, :self.n].T.copy()

    def multiply_counts(self):
        """Sizes of the owner lists of the forward products (cholamd_plan_multiply_counts): a dict per direction of items, sources and the entries
        of L one product reads."""
        out = np.zeros(6, dtype=np.int64)
        check(self.L.cholamd_plan_multiply_counts(self.h, out.ctypes.data), "cholamd_plan_multiply_counts")
        return {w: dict(items=int(out[3 * i]), sources=int(out[3 * i + 1]), entries=int(out[3 * i + 2])) for i, w in enumerate(("forward", "backward"))}

    def solve_det_host(self, arena, which, b):
        """x = M^-1 b (which = 0), M^-T b (1) or A^-1 b (-1: FORWARD then BACKWARD) on the CPU from a host arena (cholamd_plan_solve_det_host): the step
        lists of the deterministic streamed solve (Device option solve_deterministic) walked on the host.  b and the result: n doubles in original
        dof order."""
        arena = np.ascontiguousarray(arena, dtype=np.float64)
        assert arena.size == self.arena_doubles
        b = np.ascontiguousarray(b, dtype=np.float64)
        assert b.shape == (self.n,)
        x = np.full(max(self.n, 1), np.nan, dtype=np.float64)
        check(self.L.cholamd_plan_solve_det_host(self.h, arena.ctypes.data, int(which), b.ctypes.data, x.ctypes.data), "cholamd_plan_solve_det_host")
        return x[:self.n]

    def solve_det_host_nrhs(self, arena, which, B, ldb=None, ldx=None):
        """X = M^-1 B (which = 0), M^-T B (1) or A^-1 B (-1) on the CPU for the columns of B (n x k) with the step lists and the block gather's own
        partition of every source (cholamd_plan_solve_det_host_nrhs; Device option solve_deterministic_block).  ldb / ldx: leading dimensions of the
        column-major copies handed to the library (default n); the rows n .. ldx - 1 of the result are checked to be untouched.  Returns n x k.
        Deterministic and column by column independent, but not the device's bits."""
        arena = np.ascontiguousarray(arena, dtype=np.float64)
        assert arena.size == self.arena_doubles
        B = np.asarray(B, dtype=np.float64)
        assert B.ndim == 2 and B.shape[0] == self.n
        k = B.shape[1]
        ldb, ldx = int(ldb or self.n), int(ldx or self.n)
        bb = np.full((max(k, 1), max(ldb, 1)), -3.0)     # row j of the buffer = column j of B
        bb[:k, :self.n] = B.T
        xb = np.full((max(k, 1), max(ldx, 1)), np.nan)
        check(self.L.cholamd_plan_solve_det_host_nrhs(self.h, arena.ctypes.data, int(which), bb.ctypes.data, ldb, xb.ctypes.data, ldx, k), "cholamd_plan_solve_det_host_nrhs")
        assert np.isnan(xb[:, self.n:]).all(), "rows n .. ldx - 1 of X were written"
        return xb[:k, :self.n].T.copy()

    def solve_det_counts(self):
        """Sizes of the step lists of the deterministic streamed solve (cholamd_plan_solve_det_counts): a dict per direction of steps (one span launch
        each, preceded by a gather launch where the step has items), items, sources and the entries of L one sweep reads."""
        out = np.zeros(8, dtype=np.int64)
        check(self.L.cholamd_plan_solve_det_counts(self.h, out.ctypes.data), "cholamd_plan_solve_det_counts")
        return {w: dict(steps=int(out[4 * i]), items=int(out[4 * i + 1]), sources=int(out[4 * i + 2]), entries=int(out[4 * i + 3]))
                for i, w in enumerate(("forward", "backward"))}

    def solve_det_lists(self, which):
        """The lists of one direction (cholamd_plan_solve_det_lists) as int64 arrays: steps [n, 4] = level, first column of the span, first item, end
        item; items [n, 4] = first permuted position, positions, first source, end source; sources [n, 5] = arena offset, leading dimension,
        reduction steps, first permuted position read, triangle rule."""
        c = self.solve_det_counts()["forward" if which == 0 else "backward"]
        steps = np.zeros((max(c["steps"], 1), 4), dtype=np.int64)
        items = np.zeros((max(c["items"], 1), 4), dtype=np.int64)
        srcs = np.zeros((max(c["sources"], 1), 5), dtype=np.int64)
        check(self.L.cholamd_plan_solve_det_lists(self.h, int(which), steps.ctypes.data, items.ctypes.data, srcs.ctypes.data), "cholamd_plan_solve_det_lists")
        return steps[:c["steps"]], items[:c["items"]], srcs[:c["sources"]]

    @staticmethod
    def _dofs(dofs, what):
        """A dof list as the int32 array the library takes (not validated here: the library names the first offender)."""
        a = np.ascontiguousarray(np.asarray(dofs).reshape(-1), dtype=np.int32)
        if np.asarray(dofs).size and not np.array_equal(a, np.asarray(dofs).reshape(-1)):
            raise ValueError(f"{what} must be integers that fit 32 bits")
        return a

    SPARSE_COUNT_KEYS = ("separators", "steps", "items", "sources", "entries")

    @classmethod
    def _sparse_counts_dict(cls, out):
        c = {w: {k: int(out[5 * i + j]) for j, k in enumerate(cls.SPARSE_COUNT_KEYS)} for i, w in enumerate(("forward", "backward"))}
        c["positions"], c["ranges"] = int(out[10]), int(out[11])
        return c

    def sparse_counts(self, in_dofs, out_dofs):
        """Sizes of the step lists of the sparse solve pruned to up(in_dofs) (forward) and up(out_dofs) (backward) (cholamd_plan_sparse_counts): per
        direction the active separators, steps, items, sources and entries of L read -- comparable with solve_det_counts -- and the active positions
        of the union with the ranges they form."""
        i, o = self._dofs(in_dofs, "in_dofs"), self._dofs(out_dofs, "out_dofs")
        out = np.zeros(12, dtype=np.int64)
        check(self.L.cholamd_plan_sparse_counts(self.h, i.ctypes.data, i.size, o.ctypes.data, o.size, out.ctypes.data), "cholamd_plan_sparse_counts")
        return self._sparse_counts_dict(out)

    def sparse_lists(self, in_dofs, out_dofs, which):
        """The pruned lists of one direction (cholamd_plan_sparse_lists) in the formats of solve_det_lists."""
        i, o = self._dofs(in_dofs, "in_dofs"), self._dofs(out_dofs, "out_dofs")
        c = self.sparse_counts(i, o)["forward" if which == 0 else "backward"]
        steps = np.zeros((max(c["steps"], 1), 4), dtype=np.int64)
        items = np.zeros((max(c["items"], 1), 4), dtype=np.int64)
        srcs = np.zeros((max(c["sources"], 1), 5), dtype=np.int64)
        check(self.L.cholamd_plan_sparse_lists(self.h, i.ctypes.data, i.size, o.ctypes.data, o.size, int(which), steps.ctypes.data, items.ctypes.data, srcs.ctypes.data),
              "cholamd_plan_sparse_lists")
        return steps[:c["steps"]], items[:c["items"]], srcs[:c["sources"]]

    def sparse_solve_host_nrhs(self, arena, in_dofs, out_dofs, which, Bs, ldb=None, ldx=None):
        """Rows out_dofs of A^-1 b (which = -1), M^-1 b (0) or M^-T b (1) on the CPU for the columns of Bs (len(in_dofs) x k: b is Bs on in_dofs and zero
        elsewhere) with the pruned step lists (cholamd_plan_sparse_solve_host_nrhs).  ldb / ldx: leading dimensions of the column-major copies handed
        to the library (defaults: the row counts); the padding rows of the result are checked to be untouched.  Returns len(out_dofs) x k."""
        arena = np.ascontiguousarray(arena, dtype=np.float64)
        assert arena.size == self.arena_doubles
        i, o = self._dofs(in_dofs, "in_dofs"), self._dofs(out_dofs, "out_dofs")
        Bs = np.asarray(Bs, dtype=np.float64)
        assert Bs.ndim == 2 and Bs.shape[0] == i.size
        k = Bs.shape[1]
        ldb, ldx = int(ldb or max(i.size, 1)), int(ldx or max(o.size, 1))
        bb = np.full((max(k, 1), max(ldb, i.size, 1)), -3.0)     # row j of the buffer = column j of Bs
        bb[:k, :i.size] = Bs.T
        xb = np.full((max(k, 1), max(ldx, o.size, 1)), np.nan)
        check(self.L.cholamd_plan_sparse_solve_host_nrhs(self.h, arena.ctypes.data, i.ctypes.data, i.size, o.ctypes.data, o.size, int(which), bb.ctypes.data, ldb,
                                                         xb.ctypes.data, ldx, k), "cholamd_plan_sparse_solve_host_nrhs")
        assert np.isnan(xb[:, o.size:]).all(), "rows n_out .. ldx - 1 of Xs were written"
        return xb[:k, :o.size].T.copy()

    def arena_to_dense(self, arena):
        arena = np.ascontiguousarray(arena, dtype=np.float64)
        assert arena.size == self.arena_doubles
        d = np.zeros((self.n, self.n), dtype=np.float64, order="F")
        check(self.L.cholamd_plan_arena_to_dense(self.h, arena.ctypes.data, d.ctypes.data), "cholamd_plan_arena_to_dense")
        return d

    def write_matrix(self, arena, path, full_precision=False):
        arena = np.ascontiguousarray(arena, dtype=np.float64)
        check(self.L.cholamd_plan_write_matrix(self.h, arena.ctypes.data, os.fsencode(path), int(full_precision)), "cholamd_plan_write_matrix")

    def write_debug_log(self, path):
        libc = C.CDLL(None)
        libc.fopen.restype = C.c_void_p
        libc.fopen.argtypes = [C.c_char_p, C.c_char_p]
        libc.fclose.argtypes = [C.c_void_p]
        fp = libc.fopen(os.fsencode(path), b"w")
        if not fp:
            raise IOError(path)
        try:
            check(self.L.cholamd_plan_write_debug_log(self.h, fp), "cholamd_plan_write_debug_log")
        finally:
            libc.fclose(fp)


def read_vector(path, n):
    out = np.zeros(n, dtype=np.float64)
    check(load().cholamd_read_vector(os.fsencode(path), n, out.ctypes.data), "cholamd_read_vector")
    return out


def write_solution(path, x, full_precision=False):
    x = np.ascontiguousarray(x, dtype=np.float64)
    check(load().cholamd_write_solution(os.fsencode(path), x.ctypes.data, x.size, int(full_precision)), "cholamd_write_solution")


class Problem:
    """Generated Laplacian + nested-dissection ordering + clusters (cholamd_generate_laplacian)."""

    def __init__(self, nx, ny=1, nz=1, levels=3, tile=32):
        self.L = load()
        h = C.c_void_p()
        check(self.L.cholamd_generate_laplacian(nx, ny, nz, levels, tile, C.byref(h)), "cholamd_generate_laplacian")
        self.h = h
        self.n = self.L.cholamd_problem_n(h)
        self.nz = self.L.cholamd_problem_nz(h)
        self.levels = levels

    def __del__(self):
        try:
            if getattr(self, "h", None):
                self.L.cholamd_problem_destroy(self.h)
                self.h = None
        except Exception:
            pass

    def write(self, prefix):
        """<prefix>.mtx, _ord_<levels>.txt, _clust_<levels>.txt, _B.mtx in the reference's formats."""
        check(self.L.cholamd_problem_write(self.h, os.fsencode(prefix)), "cholamd_problem_write")
        lv = self.levels
        return f"{prefix}.mtx", f"{prefix}_ord_{lv}.txt", f"{prefix}_clust_{lv}.txt", f"{prefix}_B.mtx"

    def plan(self):
        h = C.c_void_p()
        check(self.L.cholamd_plan_create_from_problem(self.h, C.byref(h)), "cholamd_plan_create_from_problem")
        return Plan(_handle=h)

    def rhs(self):
        b = np.zeros(self.n, dtype=np.float64)
        self.L.cholamd_problem_rhs(self.h, b.ctypes.data)
        return b
