"""ctypes binding of libgolhip (include/golhip.h) -- the Python side of the drop-in boundary.

This is plumbing: every call goes straight to the C ABI of ``lib/libgolhip.so``, the gfx950
engine that replaces the reference's ``Broker.Publish`` -> ``GolOP.Work`` path
(broker/broker.go:157-180, server/server.go:77-107).  There is no CPU fallback: if the
library or a gfx950 device is missing, calls raise ``GolHipError``.

``import torch`` (when installed) happens before the library is loaded so that one process
never holds two HIP runtimes: torch's bundled ``libamdhip64.so`` and ``librccl.so`` carry the
same SONAMEs as /opt/rocm's, so loading torch first makes libgolhip bind to torch's copies.
"""
from __future__ import annotations

import collections
import ctypes
import os
from pathlib import Path

import numpy as np

try:  # single HIP runtime per process (see module docstring)
    import torch  # noqa: F401
except Exception:  # pragma: no cover - torch is optional for the binding itself
    torch = None

HERE = Path(__file__).resolve().parent
LIB_PATH = Path(os.environ.get("GOLHIP_LIB", HERE / "lib" / "libgolhip.so"))
# The tuning build of the same sources (-DGOLHIP_TUNING, distributed-gol_amd/Makefile): the
# production kernels plus the measured-and-rejected variants, the level-split / register-tile
# kernels and the A/B environment selectors.  Only tests of those kernels and tuning scripts load it.
TUNING_LIB_PATH = HERE / "lib_tuning" / "libgolhip.so"
FAULTS_LIB_PATH = HERE / "lib_faults" / "libgolhip.so"

OK = 0
ERR_ARG, ERR_HIP, ERR_OOM, ERR_CAP, ERR_RCCL, ERR_NODEV, ERR_STATE = -1, -2, -3, -4, -5, -6, -7
NCCL_ID_BYTES = 128
DENSITY_HALF = 0x80000000
HANDOFF_FENCED, HANDOFF_SC1 = 0, 1  # golhip_set_persistent_handoff
RECT_COPY, RECT_OR, RECT_XOR = 0, 1, 2  # golhip_load_rect
TOPOLOGY_TORUS, TOPOLOGY_PLANE = 0, 1  # golhip_batch_set_topology
_TOPOLOGIES = {"torus": TOPOLOGY_TORUS, "plane": TOPOLOGY_PLANE}
_RECT_MODES = {"copy": RECT_COPY, "or": RECT_OR, "xor": RECT_XOR}

# Every symbol include/golhip.h declares (tests/test_boundary.py checks the .so exports them).
EXPORTS = [
    "golhip_version", "golhip_strerror", "golhip_device_count", "golhip_strip_bounds",
    "golhip_halo_plan",
    "golhip_create", "golhip_create_strips", "golhip_nccl_unique_id", "golhip_create_rank",
    "golhip_comm_abort", "golhip_edge_wait", "golhip_set_activity", "golhip_activity_stats",
    "golhip_set_board_kernel", "golhip_step_persistent", "golhip_set_persistent_limit", "golhip_set_persistent_handoff",
    "golhip_create_rank_host", "golhip_destroy",
    "golhip_last_error", "golhip_get_info", "golhip_load_bytes", "golhip_init_random",
    "golhip_store_bytes", "golhip_store_words", "golhip_load_words", "golhip_step",
    "golhip_alive_count", "golhip_alive_cells", "golhip_flips", "golhip_turn",
    "golhip_set_turn", "golhip_set_k", "golhip_set_band_rows", "golhip_set_tail_bands", "golhip_sync", "golhip_timing",
    "golhip_set_graphs", "golhip_set_count_window", "golhip_set_comm_timeout",
    "golhip_kernel_time", "golhip_launch_plan", "golhip_launch_kind", "golhip_launch_kind_counts", "golhip_set_fixed_k", "golhip_track_flips",
    "golhip_step_flips", "golhip_flips_ring_capacity", "golhip_flips_fetch",
    "golhip_step_flips_rows", "golhip_flips_fetch_rows",
    "golhip_checkpoint_save", "golhip_checkpoint_load", "golhip_checkpoint_info",
    "golhip_parse_rule", "golhip_set_rule", "golhip_set_rule_masks", "golhip_get_rule",
    "golhip_store_rect", "golhip_load_rect", "golhip_view_counts", "golhip_view",
    "golhip_batch_create", "golhip_batch_destroy", "golhip_batch_last_error", "golhip_batch_load_bytes",
    "golhip_batch_store_bytes", "golhip_batch_init_random", "golhip_batch_step", "golhip_batch_alive_counts",
    "golhip_batch_track_settle", "golhip_batch_settled", "golhip_batch_turn",
    "golhip_batch_set_rule", "golhip_batch_set_rule_masks", "golhip_batch_get_rule", "golhip_batch_set_rules",
    "golhip_batch_get_rules", "golhip_batch_kernel",
    "golhip_batch_track_period", "golhip_batch_periods", "golhip_batch_search",
    "golhip_batch_search_exact",
    "golhip_batch_set_topology", "golhip_batch_get_topology", "golhip_batch_set_soup_box", "golhip_batch_get_soup_box",
    "golhip_batch_census", "golhip_batch_search_census",
    "golhip_batch_objects", "golhip_batch_search_objects",
]


class GolHipError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"golhip error {code}: {msg}")
        self.code = code


class Soup(ctypes.Structure):
    """golhip_soup_t: one soup's record of golhip_batch_search."""
    _fields_ = [("repeat_turn", ctypes.c_int64), ("period", ctypes.c_int64), ("stop_turn", ctypes.c_int64),
                ("population", ctypes.c_uint32), ("reserved", ctypes.c_uint32)]


SOUP_DTYPE = np.dtype([("repeat_turn", "<i8"), ("period", "<i8"), ("stop_turn", "<i8"), ("population", "<u4"),
                       ("reserved", "<u4")])
SEARCH_MAX_TURNS = 1 << 20


def search_stop_turn(repeat_turn: int, max_turns: int) -> int:
    """The generations Batch.search runs a soup whose first repeat is at turn repeat_turn (-1: none
    within max_turns): max_turns, or min(max_turns, 32 * ((repeat_turn - 1) // 32) + 40)."""
    return max_turns if repeat_turn < 0 else min(max_turns, 32 * ((repeat_turn - 1) // 32) + 40)


def cycle_start_floor(repeat_turn: int, period: int) -> int:
    """The lower bound on cycle_start that a soup's record alone gives, the turn from which
    Batch.search_exact compares: with s = repeat_turn - period = 2 ** j - 1 the snapshot turn,
    2 ** (j - 1) - 1 if j > 0 and period <= 2 ** (j - 1) (the previous snapshot would have matched
    within its window had the soup been on its cycle by then, so cycle_start is above it), else 0.
    Always 0 <= floor <= cycle_start <= repeat_turn - period; 0 for a record without a repeat.  The
    exact pass costs about floor + period + 2 * (cycle_start - floor) generations."""
    s = int(repeat_turn) - int(period)
    if repeat_turn < 0 or s <= 0:
        return 0
    half = (s + 1) // 2
    return half - 1 if period <= half else 0


def search_census_turn(repeat_turn: int, period: int, cycle_start: int) -> int:
    """ash_turn of Batch.search_census for a soup with this record and cycle_start: the turn of the
    board the exact pass holds when it stops.  -1 without a repeat; 0 when repeat_turn == period;
    else, with lo = cycle_start_floor(repeat_turn, period), the pass compares board(t + period) with
    board(t) from t = lo, notices the first equality (t = cycle_start) once per 32 compares and
    leaves 33 compares into that block of 32 -- at turn lo + period + 32 * ((cycle_start - lo) // 32)
    + 34 -- unless its last compare, at t = repeat_turn - period, comes first: then repeat_turn.
    Always cycle_start <= ash_turn <= repeat_turn."""
    if repeat_turn < 0:
        return -1
    s = int(repeat_turn) - int(period)
    if s <= 0:
        return 0
    lo = cycle_start_floor(repeat_turn, period)
    leave = 32 * ((int(cycle_start) - lo) // 32) + 33  # the compare behind which the pass leaves
    return lo + int(period) + leave + 1 if leave < s - lo else int(repeat_turn)


class Pattern(ctypes.Structure):
    """golhip_pattern_t: one pattern of Batch.census, h rows of w cells (1..32 each).  Bit c of alive[r]:
    cell (r, c) must be alive; bit c of care[r]: cell (r, c) is looked at (alive is a subset of care)."""
    _fields_ = [("w", ctypes.c_int32), ("h", ctypes.c_int32), ("alive", ctypes.c_uint32 * 32),
                ("care", ctypes.c_uint32 * 32)]


CENSUS_MAX_PATTERNS = 256

# what Batch.search_census returns; an output that was not asked for is None
SearchCensus = collections.namedtuple("SearchCensus", "records cycle_start ash_turn counts residue ash")


# golhip_object_t: one cluster of Batch.objects.  flags: OBJECT_WINDS_X | OBJECT_WINDS_Y | OBJECT_AT_BORDER
OBJECT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("w", "<i4"), ("h", "<i4"), ("population", "<i4"),
                         ("flags", "<u4"), ("hash", "<u8")])
OBJECT_WINDS_X, OBJECT_WINDS_Y, OBJECT_AT_BORDER = 1, 2, 4
OBJECTS_MAX = 4096

# what Batch.search_objects returns
SearchObjects = collections.namedtuple("SearchObjects", "records cycle_start ash_turn nobjects objects")

_M64 = (1 << 64) - 1


def _mix64(v: int) -> int:
    """mix(v) of include/golhip.h: the splitmix64 finaliser."""
    z = (v + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def object_hash(cells) -> int:
    """The hash Batch.objects gives a cluster of this shape that does not wind: all live (nonzero)
    cells of the 2-D array taken as ONE object, whatever their distances, in the box of their
    extent.  The same for every translation, rotation and reflection of the shape (include/golhip.h
    has the definition: the smallest over the eight orientations of the sum of mix(v << 16 | u) over
    the cells XOR mix(1 << 32 | oh << 16 | ow)).  Pure Python, no library call.  GolHipError(ERR_ARG)
    for an array that is not 2-D or has no live cell."""
    a = np.asarray(cells)
    if a.ndim != 2:
        raise GolHipError(ERR_ARG, f"object_hash: a 2-D array, not {a.ndim}-D")
    ys, xs = np.nonzero(a)
    if len(ys) == 0:
        raise GolHipError(ERR_ARG, "object_hash: no live cell")
    x0, y0 = int(xs.min()), int(ys.min())
    w, h = int(xs.max()) - x0 + 1, int(ys.max()) - y0 + 1
    place = [(int(x) - x0, int(y) - y0) for x, y in zip(xs, ys)]
    best = None
    for k in range(8):
        total = 0
        for dx, dy in place:
            fx, fy = (w - 1 - dx if k & 1 else dx), (h - 1 - dy if k & 2 else dy)
            u, v = (fx, fy) if k < 4 else (fy, fx)
            total += _mix64(v << 16 | u)
        ow, oh = (w, h) if k < 4 else (h, w)
        hk = (total & _M64) ^ _mix64(1 << 32 | oh << 16 | ow)
        best = hk if best is None or hk < best else best
    return best


def common_object_hashes() -> dict[int, str]:
    """{hash: name} of every phase of the nine objects of common_objects(): the keys under which
    Batch.objects reports them.  Orientations need no entries of their own, the hash does not change
    under them."""
    out = {}
    for name, phases in _COMMON_OBJECTS.items():
        for text in phases:
            out[object_hash(np.array([[ch == "O" for ch in row] for row in text.split("/")], dtype=np.int8))] = name
    return out


def pattern(cells) -> Pattern:
    """The Pattern of a 2-D array: 1 = the cell must be alive, 0 = it must be dead, -1 = it is not
    looked at.  GolHipError(ERR_ARG), without touching a device, for what golhip_batch_census refuses
    in a pattern: not 2-D, a side outside 1..32, a value other than 1, 0 or -1, no live cell."""
    a = np.asarray(cells)
    if a.ndim != 2:
        raise GolHipError(ERR_ARG, f"pattern: a 2-D array of 1, 0 and -1, not {a.ndim}-D")
    h, w = a.shape
    if not (1 <= w <= 32 and 1 <= h <= 32):
        raise GolHipError(ERR_ARG, f"pattern: w {w}, h {h}: 1..32 each")
    if not np.isin(a, (-1, 0, 1)).all():
        raise GolHipError(ERR_ARG, "pattern: cells are 1 (alive), 0 (dead) or -1 (not looked at)")
    if not (a == 1).any():
        raise GolHipError(ERR_ARG, "pattern: no live cell")
    p = Pattern(w=w, h=h)
    for r in range(h):
        p.alive[r] = sum(1 << c for c in range(w) if a[r, c] == 1)
        p.care[r] = sum(1 << c for c in range(w) if a[r, c] != -1)
    return p


def isolated(cells) -> np.ndarray:
    """`cells` inside a ring of dead cells, one cell wide: as a pattern it matches the object only
    where nothing touches it."""
    return np.pad(np.asarray(cells, dtype=np.int8), 1)


def orientations(cells) -> list[np.ndarray]:
    """The distinct ones of the 8 rotations and reflections of `cells`, in a fixed order: the array
    rotated by 0, 90, 180 and 270 degrees (numpy.rot90), then its left-right mirror image rotated
    the same four ways; an array equal to an earlier one is left out."""
    a = np.asarray(cells, dtype=np.int8)
    out: list[np.ndarray] = []
    for base in (a, np.fliplr(a)):
        for k in range(4):
            o = np.ascontiguousarray(np.rot90(base, k))
            if not any(o.shape == q.shape and np.array_equal(o, q) for q in out):
                out.append(o)
    return out


# the catalogue of common_objects(): every phase of each object, one orientation each
_COMMON_OBJECTS = {
    "block": ["OO/OO"],
    "beehive": [".OO./O..O/.OO."],
    "loaf": [".OO./O..O/.O.O/..O."],
    "boat": ["OO./O.O/.O."],
    "tub": [".O./O.O/.O."],
    "pond": [".OO./O..O/O..O/.OO."],
    "ship": ["OO./O.O/.OO"],
    "blinker": ["OOO"],  # its other phase is its other orientation
    "glider": [".O./..O/OOO", "O.O/.OO/.O."],  # the other two phases are mirror images of these
}


def common_objects() -> dict[str, list[np.ndarray]]:
    """The commonest ash of B3/S23 as census patterns: name -> list of int8 arrays, each the object
    inside its ring of dead cells (isolated), in every orientation and every phase.  block 1,
    beehive 2, loaf 4, boat 4, tub 1, pond 1, ship 2, blinker 2 (its two phases), glider 16 (2 phases x
    8 orientations, which hold all 4 phases): 33 arrays."""
    out = {}
    for name, phases in _COMMON_OBJECTS.items():
        arrays: list[np.ndarray] = []
        for text in phases:
            cells = np.array([[ch == "O" for ch in row] for row in text.split("/")], dtype=np.int8)
            arrays += [isolated(o) for o in orientations(cells)]
        out[name] = arrays
    return out


class Xfer(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_int32), ("peer", ctypes.c_int32), ("row", ctypes.c_int64),
                ("nrows", ctypes.c_int64)]


EXCHANGE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(Xfer), ctypes.c_int,
                               ctypes.POINTER(ctypes.c_void_p), ctypes.c_size_t)
ALLREDUCE_FN = ctypes.CFUNCTYPE(ctypes.c_int, ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64),
                                ctypes.c_size_t)


class HostCommStruct(ctypes.Structure):
    _fields_ = [("ctx", ctypes.c_void_p), ("exchange", EXCHANGE_FN), ("allreduce_u64", ALLREDUCE_FN)]


class GlooHostComm:
    """golhip_host_comm over a torch.distributed (gloo) process group: the halo exchange as
    isend/irecv of the engine's pinned host buffers in the plan's order (gloo matches the i-th send
    to a peer with that peer's i-th receive, as RCCL does inside a group), the count reduction as
    one all_reduce.  The transport for ranks that cannot use RCCL peers (several ranks on one GPU
    in the rank-mode tests: RCCL refuses a duplicate GPU)."""

    def __init__(self, group=None):
        import torch.distributed as dist

        self._dist, self._group = dist, group
        self._exchange = EXCHANGE_FN(self._do_exchange)
        self._allreduce = ALLREDUCE_FN(self._do_allreduce)
        self.struct = HostCommStruct(None, self._exchange, self._allreduce)
        self.exchanges = 0  # exchange calls seen (tests count them)
        self.reduced = []   # sizes of the count reductions seen

    def _do_exchange(self, _ctx, xfers, n, bufs, nbytes):
        try:
            reqs = []
            for i in range(n):
                x = xfers[i]
                arr = np.ctypeslib.as_array(ctypes.cast(bufs[i], ctypes.POINTER(ctypes.c_uint8)),
                                            shape=(nbytes,))
                t = torch.from_numpy(arr)
                op = self._dist.isend if x.kind == 0 else self._dist.irecv
                reqs.append(op(t, x.peer, group=self._group))
            for r in reqs:
                r.wait()
            self.exchanges += 1
            return 0
        except Exception as e:  # pragma: no cover - reported through the C ABI's error path
            print(f"golhip host transport: exchange failed: {e!r}", flush=True)
            return -1

    def _do_allreduce(self, _ctx, vals, n):
        try:
            arr = np.ctypeslib.as_array(vals, shape=(n,)).view(np.int64)
            t = torch.from_numpy(arr.copy())
            self._dist.all_reduce(t, group=self._group)  # sum; uint64 wraps like int64
            arr[:] = t.numpy()
            self.reduced.append(int(n))
            return 0
        except Exception as e:  # pragma: no cover
            print(f"golhip host transport: all_reduce failed: {e!r}", flush=True)
            return -1


class Info(ctypes.Structure):
    _fields_ = [
        ("width", ctypes.c_int64), ("height", ctypes.c_int64), ("torus_width", ctypes.c_int64),
        ("y0", ctypes.c_int64), ("rows", ctypes.c_int64), ("rank", ctypes.c_int32),
        ("world_size", ctypes.c_int32), ("nshards", ctypes.c_int32), ("k", ctypes.c_int32),
        ("halo_rows", ctypes.c_int32), ("band_rows", ctypes.c_int32),
    ]


_lib = None
_libs: dict[str, ctypes.CDLL] = {}


def load_library(path: Path | str | None = None) -> ctypes.CDLL:
    """Load libgolhip.so (raises if it was not built: no fallback).  path=None: the default library
    (GOLHIP_LIB, an alternative build for A/B experiments, else the in-tree production build);
    another path loads that build beside it (its own handle namespace, RTLD_LOCAL)."""
    global _lib
    if path is None and _lib is not None:
        return _lib
    # GOLHIP_LIB: an alternative build of the same library (A/B experiments); default in-tree
    p = Path(path) if path else Path(os.environ.get("GOLHIP_LIB", str(LIB_PATH)))
    key = str(p.resolve()) if p.exists() else str(p)
    if key in _libs:
        if path is None:
            _lib = _libs[key]
        return _libs[key]
    if not p.exists():
        raise GolHipError(ERR_NODEV, f"{p} not built (run __graft_entry__.build())")
    L = ctypes.CDLL(str(p))
    H = ctypes.c_void_p
    i64, i32, u64p = ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)
    i64p = ctypes.POINTER(ctypes.c_int64)
    sig = {
        "golhip_version": ([], i32),
        "golhip_strerror": ([i32], ctypes.c_char_p),
        "golhip_device_count": ([ctypes.POINTER(i32)], i32),
        "golhip_strip_bounds": ([i64, i32, i32, i64p, i64p], i32),
        "golhip_halo_plan": ([i64, i32, i32, i32, ctypes.POINTER(Xfer)], i32),
        "golhip_create": ([i32, i32, i32, i32, ctypes.POINTER(H)], i32),
        "golhip_create_strips": ([i32, i32, i32, i32, i32, ctypes.POINTER(H)], i32),
        "golhip_nccl_unique_id": ([ctypes.c_char_p], i32),
        "golhip_create_rank": ([i32, i32, i32, i32, i32, i32, ctypes.c_char_p, ctypes.POINTER(H)], i32),
        "golhip_create_rank_host": ([i32, i32, i32, i32, i32, i32, ctypes.POINTER(HostCommStruct),
                                     ctypes.POINTER(H)], i32),
        "golhip_destroy": ([H], i32),
        "golhip_last_error": ([H], ctypes.c_char_p),
        "golhip_get_info": ([H, ctypes.POINTER(Info)], i32),
        "golhip_load_bytes": ([H, ctypes.c_void_p, ctypes.c_size_t], i32),
        "golhip_init_random": ([H, ctypes.c_uint64, ctypes.c_uint32], i32),
        "golhip_store_bytes": ([H, ctypes.c_void_p, ctypes.c_size_t], i32),
        "golhip_store_words": ([H, ctypes.c_void_p], i32),
        "golhip_load_words": ([H, ctypes.c_void_p], i32),
        "golhip_step": ([H, i64, ctypes.c_void_p], i32),
        "golhip_step_persistent": ([H, i64, ctypes.c_void_p], i32),
        "golhip_set_persistent_limit": ([H, i32], i32),
        "golhip_set_persistent_handoff": ([H, i32], i32),
        "golhip_alive_count": ([H, u64p], i32),
        "golhip_alive_cells": ([H, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)], i32),
        "golhip_flips": ([H, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t)], i32),
        "golhip_turn": ([H, i64p], i32),
        "golhip_set_turn": ([H, i64], i32),
        "golhip_set_k": ([H, i32], i32),
        "golhip_set_band_rows": ([H, i32], i32),
        "golhip_set_tail_bands": ([H, i32, i32], i32),
        "golhip_set_fixed_k": ([H, i32], i32),
        "golhip_track_flips": ([H, i32], i32),
        "golhip_checkpoint_save": ([H, ctypes.c_char_p], i32),
        "golhip_checkpoint_load": ([H, ctypes.c_char_p], i32),
        "golhip_checkpoint_info": ([ctypes.c_char_p, i64p, i64p, i64p], i32),
        "golhip_step_flips": ([H, i64, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                               ctypes.c_void_p, ctypes.c_void_p], i32),
        "golhip_flips_ring_capacity": ([H, i64p], i32),
        "golhip_flips_fetch": ([H, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                ctypes.c_void_p], i32),
        "golhip_step_flips_rows": ([H, i64, ctypes.c_void_p, ctypes.c_size_t,
                                    ctypes.POINTER(ctypes.c_size_t), ctypes.c_void_p, ctypes.c_void_p], i32),
        "golhip_flips_fetch_rows": ([H, ctypes.c_void_p, ctypes.c_size_t, ctypes.POINTER(ctypes.c_size_t),
                                     ctypes.c_void_p], i32),
        "golhip_sync": ([H], i32),
        "golhip_set_graphs": ([H, i32], i32),
        "golhip_set_count_window": ([H, i32], i32),
        "golhip_set_comm_timeout": ([H, i64], i32),
        "golhip_comm_abort": ([H], i32),
        "golhip_timing": ([H, i32], i32),
        "golhip_kernel_time": ([H, ctypes.POINTER(ctypes.c_double), i64p, i64p], i32),
        "golhip_edge_wait": ([H, ctypes.POINTER(ctypes.c_double), i64p], i32),
        "golhip_set_activity": ([H, i32], i32),
        "golhip_set_board_kernel": ([H, i32], i32),
        "golhip_activity_stats": ([H, i64p, i64p], i32),
        "golhip_launch_plan": ([i64, i64, i32, i32, i64, ctypes.c_void_p, ctypes.c_size_t,
                                ctypes.POINTER(ctypes.c_size_t)], i32),
        "golhip_parse_rule": ([ctypes.c_char_p, ctypes.POINTER(ctypes.c_uint32),
                               ctypes.POINTER(ctypes.c_uint32)], i32),
        "golhip_set_rule": ([H, ctypes.c_char_p], i32),
        "golhip_set_rule_masks": ([H, ctypes.c_uint32, ctypes.c_uint32], i32),
        "golhip_get_rule": ([H, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)], i32),
        "golhip_store_rect": ([H, i64, i64, i64, i64, ctypes.c_void_p, ctypes.c_size_t], i32),
        "golhip_load_rect": ([H, i64, i64, i64, i64, ctypes.c_void_p, ctypes.c_size_t, i32], i32),
        "golhip_view_counts": ([H, i64, i64, i64, i64, i32, ctypes.c_void_p], i32),
        "golhip_view": ([H, i64, i64, i64, i64, i32, ctypes.c_void_p, ctypes.c_size_t], i32),
        "golhip_launch_kind": ([H, i32, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)], i32),
        "golhip_batch_create": ([i32, i32, i32, i32, ctypes.POINTER(H)], i32),
        "golhip_batch_destroy": ([H], i32),
        "golhip_batch_last_error": ([H], ctypes.c_char_p),
        "golhip_batch_load_bytes": ([H, i32, i32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t], i32),
        "golhip_batch_store_bytes": ([H, i32, i32, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_size_t], i32),
        "golhip_batch_init_random": ([H, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32], i32),
        "golhip_batch_step": ([H, i64, ctypes.c_void_p, ctypes.c_size_t], i32),
        "golhip_batch_alive_counts": ([H, ctypes.c_void_p], i32),
        "golhip_batch_track_settle": ([H, i32], i32),
        "golhip_batch_settled": ([H, ctypes.c_void_p], i32),
        "golhip_batch_track_period": ([H, i32], i32),
        "golhip_batch_periods": ([H, ctypes.c_void_p, ctypes.c_void_p], i32),
        "golhip_batch_search": ([H, i64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, i64, ctypes.c_void_p,
                                 ctypes.c_void_p, ctypes.c_void_p], i32),
        "golhip_batch_search_exact": ([H, i64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, i64,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], i32),
        "golhip_batch_turn": ([H, i64p], i32),
        "golhip_batch_set_rule": ([H, ctypes.c_char_p], i32),
        "golhip_batch_set_rule_masks": ([H, ctypes.c_uint32, ctypes.c_uint32], i32),
        "golhip_batch_get_rule": ([H, ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(ctypes.c_uint32)], i32),
        "golhip_batch_set_rules": ([H, ctypes.c_void_p, ctypes.c_void_p], i32),
        "golhip_batch_get_rules": ([H, ctypes.c_void_p, ctypes.c_void_p], i32),
        "golhip_batch_kernel": ([H, ctypes.POINTER(i32)], i32),
        "golhip_batch_set_topology": ([H, i32], i32),
        "golhip_batch_get_topology": ([H, ctypes.POINTER(i32)], i32),
        "golhip_batch_set_soup_box": ([H, i32, i32], i32),
        "golhip_batch_get_soup_box": ([H, ctypes.POINTER(i32), ctypes.POINTER(i32)], i32),
        "golhip_batch_census": ([H, ctypes.c_void_p, i32, ctypes.c_void_p, ctypes.c_void_p], i32),
        "golhip_batch_search_census": ([H, i64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, i64,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, i32, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p], i32),
        "golhip_batch_objects": ([H, i32, i32, ctypes.c_void_p, ctypes.c_void_p], i32),
        "golhip_batch_search_objects": ([H, i64, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_uint32, i64,
                                         ctypes.c_void_p, ctypes.c_void_p, i32, i32, ctypes.c_void_p, ctypes.c_void_p,
                                         ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p], i32),
        "golhip_launch_kind_counts": ([H, i32, i32, ctypes.POINTER(ctypes.c_int),
                                       ctypes.POINTER(ctypes.c_int)], i32),
    }
    for name, (args, res) in sig.items():
        f = getattr(L, name)
        f.argtypes = args
        f.restype = res
    _libs[key] = L
    if path is None:
        _lib = L
    if _default_comm_timeout_ms is not None:  # set_default_comm_timeout reaches every library
        L.golhip_set_comm_timeout(None, _default_comm_timeout_ms)
    return L


def tuning_library() -> ctypes.CDLL:
    """The tuning build (lib_tuning/libgolhip.so): pass it as Engine(..., lib=tuning_library()) to
    run a non-production kernel (GOLHIP_VARIANT / GOLHIP_SPLIT / GOLHIP_TILE / GOLHIP_SLAB ...).
    Built here; pushed to a GPU box only for the runs that load it (.gpurunignore)."""
    return load_library(TUNING_LIB_PATH)


def fault_library() -> ctypes.CDLL:
    """The production kernels + the tuning library's engine hooks (lib_faults/libgolhip.so): fault
    injection (GOLHIP_FAULT) and the A/B selectors over the production kernels -- what the fail-fast
    tests load."""
    return load_library(FAULTS_LIB_PATH)


_default_comm_timeout_ms: int | None = None


def set_default_comm_timeout(ms: int, lib: ctypes.CDLL | None = None) -> None:
    """golhip_set_comm_timeout(NULL, ms): the RCCL deadline of engines created from now on, in every
    library loaded now or later (an Engine(..., lib=tuning_library()) in rank mode included), or
    only in `lib` when given."""
    global _default_comm_timeout_ms
    if int(ms) <= 0:
        raise GolHipError(ERR_ARG, "set_comm_timeout: invalid argument")
    if lib is not None:
        libs = [lib]
    else:
        _default_comm_timeout_ms = int(ms)
        libs = list(_libs.values()) or [load_library()]
    for L in libs:
        rc = L.golhip_set_comm_timeout(None, int(ms))
        if rc != OK:
            raise GolHipError(rc, "set_comm_timeout: invalid argument")


class _CallLog:
    """The library seen through an engine: records the name of the last C ABI function called
    (Engine.last_call), so a failed or stuck multi-rank run can say where it was."""

    def __init__(self, lib: ctypes.CDLL, owner: "Engine"):
        self._lib, self._owner = lib, owner

    _QUIET = ("golhip_last_error", "golhip_strerror", "golhip_get_info")

    def __getattr__(self, name):
        if name not in self._QUIET:
            self._owner.last_call = name
        return getattr(self._lib, name)


def parse_rle(text: str) -> np.ndarray:
    """Run-length-encoded Life pattern (the standard .rle format) -> 0/255 uint8 (h, w)."""
    lines = [ln.strip() for ln in text.splitlines() if ln.strip() and not ln.startswith("#")]
    header, body = lines[0], "".join(lines[1:])
    dims = dict(kv.split("=") for kv in header.replace(" ", "").split(",")[:2])
    w, h = int(dims["x"]), int(dims["y"])
    out = np.zeros((h, w), dtype=np.uint8)
    x = y = 0
    run = ""
    for ch in body:
        if ch.isdigit():
            run += ch
            continue
        n = int(run) if run else 1
        run = ""
        if ch == "b":
            x += n
        elif ch == "o":
            out[y, x:x + n] = 255
            x += n
        elif ch == "$":
            y += n
            x = 0
        elif ch == "!":
            break
    return out


def place(board: np.ndarray, pattern: np.ndarray, x: int, y: int) -> None:
    """Stamp a pattern at (x, y) on a torus board (in place)."""
    h, w = pattern.shape
    H, W = board.shape
    ys = (np.arange(h) + y) % H
    xs = (np.arange(w) + x) % W
    board[np.ix_(ys, xs)] |= pattern


def pinned_empty(shape, dtype) -> np.ndarray:
    """A page-locked host array when a GPU is present (device -> host copies into it are one DMA at
    the full PCIe rate instead of going through the runtime's pageable staging), else a plain one.
    The array keeps its torch storage alive."""
    if torch is not None and torch.cuda.is_available():
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        t = torch.empty(max(n, 1), dtype=torch.uint8, pin_memory=True)
        a = t.numpy()[:n].view(dtype).reshape(shape)
        return a
    return np.zeros(shape, dtype=dtype)


def device_count() -> int:
    n = ctypes.c_int(0)
    load_library().golhip_device_count(ctypes.byref(n))
    return n.value


def strip_bounds(height: int, world_size: int, rank: int) -> tuple[int, int]:
    """Rows [y0, y0+rows) of `rank` (pure host arithmetic, no device)."""
    y0, rows = ctypes.c_int64(), ctypes.c_int64()
    rc = load_library().golhip_strip_bounds(height, world_size, rank, ctypes.byref(y0), ctypes.byref(rows))
    if rc != OK:
        raise GolHipError(rc, "strip_bounds: invalid arguments")
    return y0.value, rows.value


def halo_plan(height: int, world_size: int, rank: int, k: int) -> list[tuple[str, int, int, int]]:
    """The engine's 4 halo transfers for `rank`, in issue order: (send|recv, peer, row, nrows)."""
    arr = (Xfer * 4)()
    rc = load_library().golhip_halo_plan(height, world_size, rank, k, arr)
    if rc != OK:
        raise GolHipError(rc, "halo_plan: invalid arguments")
    return [("send" if x.kind == 0 else "recv", x.peer, x.row, x.nrows) for x in arr]


def launch_plan(width: int, height: int, k: int, turns: int, strips: int = 1) -> list[int]:
    """The launch depths golhip_step(turns) runs (pure host arithmetic, no device): > 0 one
    stencil launch of that depth, < 0 one graph replay of that many generations."""
    L = load_library()
    n = ctypes.c_size_t(0)
    rc = L.golhip_launch_plan(width, height, strips, k, turns, None, 0, ctypes.byref(n))
    if rc != OK:
        raise GolHipError(rc, "launch_plan: invalid arguments")
    out = np.zeros(max(n.value, 1), dtype=np.int32)
    rc = L.golhip_launch_plan(width, height, strips, k, turns, out.ctypes.data, n.value, ctypes.byref(n))
    if rc != OK:
        raise GolHipError(rc, "launch_plan failed")
    return [int(x) for x in out[: n.value]]


def parse_rule(text: str | bytes | None, lib: ctypes.CDLL | None = None) -> tuple[int, int]:
    """"B36/S23" -> (birth, survive) masks: bit n of birth = a dead cell with n live neighbours is
    born, bit n of survive = a live cell with n live neighbours stays alive (pure host, no device)."""
    L = lib if lib is not None else load_library()
    b, s = ctypes.c_uint32(), ctypes.c_uint32()
    raw = text.encode() if isinstance(text, str) else text
    rc = L.golhip_parse_rule(raw, ctypes.byref(b), ctypes.byref(s))
    if rc != OK:
        raise GolHipError(rc, L.golhip_last_error(None).decode() or f"bad rule {text!r}")
    return b.value, s.value


def rule_string(birth: int, survive: int) -> str:
    """The canonical text of a rule's masks: digits ascending, "B36/S23"."""
    digits = lambda m: "".join(str(n) for n in range(9) if (m >> n) & 1)  # noqa: E731
    return f"B{digits(birth)}/S{digits(survive)}"


def checkpoint_info(path) -> tuple[int, int, int]:
    """(width, height, turn) of a checkpoint file (pure host, no device)."""
    w, h, t = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    rc = load_library().golhip_checkpoint_info(str(path).encode(), ctypes.byref(w), ctypes.byref(h),
                                               ctypes.byref(t))
    if rc != OK:
        raise GolHipError(rc, f"{path}: not a golhip checkpoint")
    return w.value, h.value, t.value


def nccl_unique_id() -> bytes:
    buf = ctypes.create_string_buffer(NCCL_ID_BYTES)
    rc = load_library().golhip_nccl_unique_id(buf)
    if rc != OK:
        raise GolHipError(rc, "ncclGetUniqueId failed")
    return buf.raw


class Engine:
    """One libgolhip handle.  Mirrors the broker's role: the board lives on the GPU(s)."""

    def __init__(self, width: int, height: int, ngpus: int = 1, k: int = 1, *, rank: int | None = None,
                 world_size: int = 1, device: int = 0, nccl_id: bytes | None = None,
                 strips: int | None = None, host_comm: GlooHostComm | None = None,
                 lib: ctypes.CDLL | None = None, rule: str | tuple[int, int] | None = None):
        self.last_call = "golhip_create"
        L = _CallLog(lib if lib is not None else load_library(), self)
        self._L = L
        self._h = ctypes.c_void_p()
        self.host_comm = host_comm  # keeps the ctypes callbacks alive with the handle
        if host_comm is not None:
            rc = L.golhip_create_rank_host(width, height, rank or 0, world_size, device, k,
                                           ctypes.byref(host_comm.struct), ctypes.byref(self._h))
        elif strips is not None:
            rc = L.golhip_create_strips(width, height, strips, ngpus, k, ctypes.byref(self._h))
        elif rank is None:
            rc = L.golhip_create(width, height, ngpus, k, ctypes.byref(self._h))
        else:
            rc = L.golhip_create_rank(width, height, rank, world_size, device, k, nccl_id,
                                      ctypes.byref(self._h))
        if rc != OK:
            why = L.golhip_last_error(None).decode() or L.golhip_strerror(rc).decode()
            raise GolHipError(rc, why)
        self.info = self.get_info()
        if rule is not None:  # default: B3/S23
            try:
                self.set_rule(rule)
            except Exception:
                self.close()
                raise

    # -- plumbing
    def _check(self, rc: int) -> int:
        if rc != OK:
            raise GolHipError(rc, self._L.golhip_last_error(self._h).decode() or
                              self._L.golhip_strerror(rc).decode())
        return rc

    def close(self):
        if self._h:
            self._L.golhip_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def get_info(self) -> Info:
        info = Info()
        self._check(self._L.golhip_get_info(self._h, ctypes.byref(info)))
        return info

    # -- board in/out
    def load(self, cells: np.ndarray):
        cells = np.ascontiguousarray(cells, dtype=np.uint8)
        assert cells.shape == (self.info.rows, self.info.width), cells.shape
        self._check(self._L.golhip_load_bytes(self._h, cells.ctypes.data, cells.strides[0]))

    def init_random(self, seed: int, density_q32: int = DENSITY_HALF):
        self._check(self._L.golhip_init_random(self._h, seed, density_q32))

    def store(self) -> np.ndarray:
        out = np.empty((self.info.rows, self.info.width), dtype=np.uint8)
        self._check(self._L.golhip_store_bytes(self._h, out.ctypes.data, out.strides[0]))
        return out

    def store_words(self) -> np.ndarray:
        out = np.empty((self.info.rows, self.info.width // 64), dtype=np.uint64)
        self._check(self._L.golhip_store_words(self._h, out.ctypes.data))
        return out

    def load_words(self, words: np.ndarray):
        words = np.ascontiguousarray(words, dtype=np.uint64)
        assert words.shape == (self.info.rows, self.info.width // 64)
        self._check(self._L.golhip_load_words(self._h, words.ctypes.data))

    # -- windowed access (global coordinates, any int, wrapping round the torus)
    def store_rect(self, x: int, y: int, w: int, h: int) -> np.ndarray:
        """golhip_store_rect: the w x h rectangle whose top-left cell is (x, y), 0/255 uint8 (h, w)."""
        out = np.empty((max(h, 0), max(w, 0)), dtype=np.uint8)
        self._check(self._L.golhip_store_rect(self._h, x, y, w, h, out.ctypes.data, max(w, 0)))
        return out

    def load_rect(self, x: int, y: int, cells: np.ndarray, mode: str | int = "copy"):
        """golhip_load_rect: write 0/nonzero `cells` (h, w) into the running board at (x, y) --
        mode "copy" / "or" / "xor" (or RECT_*).  The turn is kept."""
        cells = np.ascontiguousarray(cells, dtype=np.uint8)
        assert cells.ndim == 2, cells.shape
        m = _RECT_MODES[mode] if isinstance(mode, str) else int(mode)
        self._check(self._L.golhip_load_rect(self._h, x, y, cells.shape[1], cells.shape[0],
                                             cells.ctypes.data, cells.strides[0], m))

    def place(self, pattern: np.ndarray, x: int, y: int, mode: str | int = "or"):
        """Stamp a pattern (parse_rle's 0/255 array) at (x, y) on the device board: the module's
        place() for the running board, without reloading it."""
        self.load_rect(x, y, pattern, mode)

    def view_counts(self, x: int, y: int, w: int, h: int, scale: int, out: np.ndarray | None = None) -> np.ndarray:
        """golhip_view_counts: uint32 (h, w), pixel (j, i) = live cells of the scale x scale block
        whose top-left cell is (x + i*scale, y + j*scale).  out: a C-contiguous uint32 (h, w) array to
        fill instead of a new one (a display loop reuses one, page-locked: pinned_empty)."""
        if out is None:
            out = np.empty((max(h, 0), max(w, 0)), dtype=np.uint32)
        assert out.dtype == np.uint32 and out.shape == (h, w) and out.flags.c_contiguous
        self._check(self._L.golhip_view_counts(self._h, x, y, w, h, scale, out.ctypes.data))
        return out

    def view(self, x: int, y: int, w: int, h: int, scale: int) -> np.ndarray:
        """golhip_view: the viewport as grey uint8 (h, w), ceil(255 * count / scale^2)."""
        out = np.empty((max(h, 0), max(w, 0)), dtype=np.uint8)
        self._check(self._L.golhip_view(self._h, x, y, w, h, scale, out.ctypes.data, max(w, 0)))
        return out

    # -- the rule
    def set_rule(self, rule: str | tuple[int, int]):
        """golhip_set_rule: "B36/S23" or (birth, survive) masks.  Keeps the board, the turn and every
        setting; B3/S23 runs the production kernels, any other rule the rule-generic kernel
        (launch_kind: "rule").  A checkpoint does not hold the rule: set it again after loading."""
        if isinstance(rule, (str, bytes)):
            self._check(self._L.golhip_set_rule(self._h, rule.encode() if isinstance(rule, str) else rule))
        else:
            birth, survive = rule
            self._check(self._L.golhip_set_rule_masks(self._h, int(birth), int(survive)))

    def set_rule_masks(self, birth: int, survive: int):
        self.set_rule((birth, survive))

    @property
    def rule_masks(self) -> tuple[int, int]:
        b, s = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._L.golhip_get_rule(self._h, ctypes.byref(b), ctypes.byref(s)))
        return b.value, s.value

    @property
    def rule(self) -> str:
        """The handle's rule in canonical form, e.g. "B36/S23"."""
        return rule_string(*self.rule_masks)

    # -- hot path
    def step(self, turns: int, counts: bool = False) -> np.ndarray | None:
        if counts:
            out = np.zeros(max(turns, 1), dtype=np.uint64)
            self._check(self._L.golhip_step(self._h, turns, out.ctypes.data))
            return out[:turns]
        self._check(self._L.golhip_step(self._h, turns, None))
        return None

    def step_persistent(self, turns: int) -> np.ndarray:
        """golhip_step_persistent: `turns` turns with every count, one persistent-slab launch per
        count window (opt-in; configs[1] / configs[4]-like boards).  Refuses (GOLHIP_ERR_STATE,
        board unchanged) when the slabs cannot all be resident; restores the board on a timeout."""
        out = np.zeros(max(turns, 1), dtype=np.uint64)
        self._check(self._L.golhip_step_persistent(self._h, turns, out.ctypes.data))
        return out[:turns]

    def set_persistent_handoff(self, mode: int) -> None:
        """golhip_set_persistent_handoff: HANDOFF_FENCED (default) or HANDOFF_SC1 (measured form)."""
        self._check(self._L.golhip_set_persistent_handoff(self._h, mode))

    def set_persistent_limit(self, max_groups: int) -> None:
        """golhip_set_persistent_limit: slabs the caller owns CUs for (0 = the whole device)."""
        self._check(self._L.golhip_set_persistent_limit(self._h, max_groups))

    def alive_count(self) -> int:
        v = ctypes.c_uint64()
        self._check(self._L.golhip_alive_count(self._h, ctypes.byref(v)))
        return v.value

    def _cells(self, fn) -> np.ndarray:
        n = ctypes.c_size_t(0)
        rc = fn(self._h, None, 0, ctypes.byref(n))
        if rc not in (OK, ERR_CAP):
            self._check(rc)
        out = np.empty((max(n.value, 1), 2), dtype=np.int32)
        self._check(fn(self._h, out.ctypes.data, n.value, ctypes.byref(n)))
        return out[: n.value]

    def alive_cells(self) -> np.ndarray:
        """(n, 2) int32 array of (x, y), row-major (gol/distributor.go:153-166)."""
        return self._cells(self._L.golhip_alive_cells)

    def flips(self) -> np.ndarray:
        """(n, 2) int32 array of (x, y) that changed in the last generation."""
        return self._cells(self._L.golhip_flips)

    def checkpoint_save(self, path):
        self._check(self._L.golhip_checkpoint_save(self._h, str(path).encode()))

    def checkpoint_load(self, path):
        self._check(self._L.golhip_checkpoint_load(self._h, str(path).encode()))

    def track_flips(self, enable: bool = True):
        """Keep the last generation's flips on every step (golhip_flips valid after a K-deep step)."""
        self._check(self._L.golhip_track_flips(self._h, int(enable)))

    def flips_ring_capacity(self) -> int:
        v = ctypes.c_int64()
        self._check(self._L.golhip_flips_ring_capacity(self._h, ctypes.byref(v)))
        return v.value

    def step_flips(self, turns: int, counts: bool = False):
        """Advance `turns` keeping every turn's flips: returns (list of per-turn (n_t, 2) views of
        a host buffer reused by the next call, alive counts per turn or None)."""
        n = ctypes.c_size_t(0)
        per = np.zeros(max(turns, 1), dtype=np.uint64)
        alive = np.zeros(max(turns, 1), dtype=np.uint64) if counts else None
        # one page-locked host list reused across calls (a fresh multi-100-MB array per call would
        # spend its time in page faults; pageable memory halves the copy rate): filled directly
        # when it fits, else grown and fetched
        buf = getattr(self, "_flip_buf", None)
        if buf is None:
            buf = self._flip_buf = pinned_empty((1 << 16, 2), np.int32)
        rc = self._L.golhip_step_flips(self._h, turns, buf.ctypes.data, len(buf), ctypes.byref(n),
                                       per.ctypes.data, alive.ctypes.data if counts else None)
        if rc == ERR_CAP:
            buf = self._flip_buf = pinned_empty((max(n.value, 2 * len(buf)), 2), np.int32)
            self._check(self._L.golhip_flips_fetch(self._h, buf.ctypes.data, len(buf),
                                                   ctypes.byref(n), per.ctypes.data))
        else:
            self._check(rc)
        xy = buf
        bounds = np.concatenate([[0], np.cumsum(per[:turns])]).astype(np.int64)
        out = [xy[bounds[t]:bounds[t + 1]] for t in range(turns)]
        return out, (alive[:turns] if counts else None)

    def step_flips_rows(self, turns: int, counts: bool = False):
        """golhip_step_flips_rows: (x, row_offsets, alive counts or None), views of page-locked
        buffers reused by the next call.  x[row_offsets[t*rows + y] : row_offsets[t*rows + y + 1]]
        are the x of the cells turn t flipped on row y of this handle's strip."""
        n = ctypes.c_size_t(0)
        rows = self.info.rows
        alive = np.zeros(max(turns, 1), dtype=np.uint64) if counts else None
        offs = getattr(self, "_rows_offs", None)
        if offs is None or len(offs) < turns * rows + 1:
            offs = self._rows_offs = pinned_empty((turns * rows + 1,), np.uint64)
        x = getattr(self, "_rows_x", None)
        if x is None:
            x = self._rows_x = pinned_empty((1 << 17,), np.uint16)
        rc = self._L.golhip_step_flips_rows(self._h, turns, x.ctypes.data, len(x), ctypes.byref(n),
                                            offs.ctypes.data, alive.ctypes.data if counts else None)
        if rc == ERR_CAP:
            x = self._rows_x = pinned_empty((max(n.value, 2 * len(x)),), np.uint16)
            self._check(self._L.golhip_flips_fetch_rows(self._h, x.ctypes.data, len(x), ctypes.byref(n),
                                                        offs.ctypes.data))
        else:
            self._check(rc)
        return x[:n.value], offs[:turns * rows + 1], (alive[:turns] if counts else None)

    @staticmethod
    def rows_to_cells(x, offs, rows: int, turns: int, y0: int = 0):
        """Expand golhip_step_flips_rows output to per-turn (n_t, 2) int32 (x, y) arrays (tests)."""
        out = []
        for t in range(turns):
            o = offs[t * rows:(t + 1) * rows + 1].astype(np.int64)
            ys = np.repeat(np.arange(rows, dtype=np.int32) + y0, np.diff(o))
            xs = x[o[0]:o[-1]].astype(np.int32)
            out.append(np.stack([xs, ys], axis=1) if len(xs) else np.zeros((0, 2), np.int32))
        return out

    @property
    def turn(self) -> int:
        t = ctypes.c_int64()
        self._check(self._L.golhip_turn(self._h, ctypes.byref(t)))
        return t.value

    @turn.setter
    def turn(self, value: int):
        self._check(self._L.golhip_set_turn(self._h, value))

    # -- tuning / measurement
    def set_k(self, k: int):
        self._check(self._L.golhip_set_k(self._h, k))
        self.info = self.get_info()

    def set_fixed_k(self, fixed: bool):
        """Every bulk launch exactly k deep (depth sweeps); default: fastest measured depth <= k."""
        self._check(self._L.golhip_set_fixed_k(self._h, int(fixed)))

    def set_band_rows(self, rows: int):
        self._check(self._L.golhip_set_band_rows(self._h, rows))
        self.info = self.get_info()

    def set_tail_bands(self, bands: int, rows: int):
        self._check(self._L.golhip_set_tail_bands(self._h, bands, rows))

    def set_graphs(self, mode: int):
        """Graph replay of step blocks: -1 automatic, 0 never, 1 whenever the plan allows."""
        self._check(self._L.golhip_set_graphs(self._h, mode))

    def set_count_window(self, generations: int):
        self._check(self._L.golhip_set_count_window(self._h, generations))

    def set_comm_timeout(self, ms: int):
        """Deadline of waits on RCCL-dependent work (rank mode): ERR_RCCL when it passes."""
        self._check(self._L.golhip_set_comm_timeout(self._h, int(ms)))

    def comm_abort(self):
        """After GOLHIP_ERR_RCCL: ncclCommAbort the handle's communicator (RCCL aborts its operations
        still running on the device), so the streams can drain before close()."""
        self._check(self._L.golhip_comm_abort(self._h))

    def launch_kind(self, k: int, counts: bool = False) -> tuple[str, int]:
        """The kernel a k-deep launch runs (with / without per-generation counts): ("stream", 0),
        ("split", S), ("tile", T), ("slab", [10000 NC +] 100 W + S), ("board", 100 W + R) or, for
        any rule but B3/S23, ("rule", 1 constant-folded / 0 table form)."""
        kind, param = ctypes.c_int(), ctypes.c_int()
        self._check(self._L.golhip_launch_kind_counts(self._h, k, int(counts), ctypes.byref(kind),
                                                      ctypes.byref(param)))
        return ("stream", "split", "tile", "slab", "board", "rule")[kind.value], param.value

    def sync(self):
        self._check(self._L.golhip_sync(self._h))

    def timing(self, enable: bool):
        self._check(self._L.golhip_timing(self._h, int(enable)))

    def set_activity(self, enable: int):
        """Stable-slab skipping of the slab launches (golhip_set_activity): -1 automatic (the
        default: boards with more slabs than CUs), 0 / False off, 1 / True on."""
        self._check(self._L.golhip_set_activity(self._h, int(enable)))

    def set_board_kernel(self, enable: int):
        """The whole-board kernel for boards that fit one workgroup (golhip_set_board_kernel): -1
        automatic (the default: boards of at most 256 rows), 0 / False off, 1 / True every board
        it fits."""
        self._check(self._L.golhip_set_board_kernel(self._h, int(enable)))

    def activity_stats(self) -> tuple[int, int]:
        """(slabs computed, slabs skipped) since create (golhip_activity_stats)."""
        c, k = ctypes.c_int64(), ctypes.c_int64()
        self._check(self._L.golhip_activity_stats(self._h, ctypes.byref(c), ctypes.byref(k)))
        return c.value, k.value

    def edge_wait(self) -> tuple[float, int]:
        """With timing on (split boards): ms the compute stream waited for the boundary bands after
        each block's interior, summed, and the number of blocks (golhip_edge_wait)."""
        ms, blocks = ctypes.c_double(), ctypes.c_int64()
        self._check(self._L.golhip_edge_wait(self._h, ctypes.byref(ms), ctypes.byref(blocks)))
        return ms.value, blocks.value

    def kernel_time(self) -> tuple[float, int, int]:
        ms, launches, gens = ctypes.c_double(), ctypes.c_int64(), ctypes.c_int64()
        self._check(self._L.golhip_kernel_time(self._h, ctypes.byref(ms), ctypes.byref(launches),
                                               ctypes.byref(gens)))
        return ms.value, launches.value, gens.value


class Batch:
    """One golhip_batch handle: `nboards` independent tori of one small size on one device, all
    advanced by one launch (one workgroup per board).  Sizes: widths whose lcm with 128 is 128, 256
    or 512 (16, 64, 128, 256, 512, ...) and 4, 8, 16, ..., 512 rows.  The batch has one turn counter;
    any load() or init_random() sets it to 0 and clears the settle and period records.

    The rule is B3/S23 unless `rule` ("B36/S23" or (birth, survive) masks: one life-like rule for all
    boards) or `rules` (one per board) is given, or set later with set_rule() / set_rules().  A
    uniform B3/S23 runs gol_batch; any other rule runs gol_batch_rule, constant-folded for a uniform
    catalogue rule, in the table form otherwise -- per-board rules always (kernel_form).  Rule texts
    and the length of `rules` are checked before the handle is created: a bad one raises
    GolHipError(ERR_ARG) naming it, without touching a device.

    topology: "torus" (the default) or "plane", a bounded grid whose outside is dead (set_topology,
    topology).  soup_box: (w, h), the centred box outside which init_random and search clear every
    cell of a soup, or None for the whole board (set_soup_box, soup_box).

    Soups: search() runs seeds, not boards of the batch, each until it repeats; search_exact() adds
    every soup's cycle_start, the exact turn at which it enters its cycle.  census() says what the
    boards hold: per board, how often each pattern of a list matches and how many live cells no match
    explains.  search_census() is search_exact() with that census of each soup's ash, no boards kept."""

    def __init__(self, width: int, height: int, nboards: int, device: int = 0, *,
                 rule: str | tuple[int, int] | None = None, rules=None, topology: str | int = "torus",
                 soup_box: tuple[int, int] | None = None, lib: ctypes.CDLL | None = None):
        self._L = lib if lib is not None else load_library()
        self._h = ctypes.c_void_p()
        masks = None if rule is None else self._masks_of(rule)
        pairs = None if rules is None else self._pairs_of(rules, int(nboards))
        topo = self._topology_of(topology)
        rc = self._L.golhip_batch_create(width, height, nboards, device, ctypes.byref(self._h))
        if rc != OK:
            why = self._L.golhip_batch_last_error(None).decode() or self._L.golhip_strerror(rc).decode()
            raise GolHipError(rc, why)
        self.width, self.height, self.nboards = int(width), int(height), int(nboards)
        if masks is not None:
            self.set_rule(masks)
        if pairs is not None:
            self.set_rules(pairs)
        try:
            if topo != TOPOLOGY_TORUS:
                self.set_topology(topo)
            if soup_box is not None:
                self.set_soup_box(soup_box)
        except GolHipError:
            self.close()
            raise

    @staticmethod
    def _topology_of(topology) -> int:
        """The C value of "torus" / "plane"; an integer passes through for the library to check."""
        if isinstance(topology, str):
            if topology not in _TOPOLOGIES:
                raise GolHipError(ERR_ARG, f"topology {topology!r}: \"torus\" or \"plane\"")
            return _TOPOLOGIES[topology]
        return int(topology)

    def _masks_of(self, rule, where: str = "") -> tuple[int, int]:
        """(birth, survive) of a rule text or a pair of masks; GolHipError(ERR_ARG) naming a bad one."""
        try:
            if isinstance(rule, (str, bytes)):
                return parse_rule(rule, self._L)
            birth, survive = (int(v) for v in rule)
            if birth < 0 or survive < 0 or (birth | survive) & ~0x1FF:
                raise GolHipError(ERR_ARG, f"rule masks birth={birth:#x} survive={survive:#x}: bits above 8 "
                                           "(a cell has 8 neighbours)")
            return birth, survive
        except GolHipError as e:
            raise GolHipError(e.code, where + str(e).split(": ", 1)[1]) if where else e
        except (TypeError, ValueError):
            raise GolHipError(ERR_ARG, f"{where}rule {rule!r}: a text like \"B36/S23\" or (birth, survive) masks")

    def _pairs_of(self, rules, nboards: int) -> np.ndarray:
        """An (nboards, 2) uint32 array of masks from a sequence of rule texts or (birth, survive) pairs,
        or an (nboards, 2) integer array."""
        n = len(rules)
        if n != nboards:
            raise GolHipError(ERR_ARG, f"rules: {n} rules for {nboards} boards")
        return np.array([self._masks_of(r, f"rules[{i}]: ") for i, r in enumerate(rules)],
                        dtype=np.uint32).reshape(nboards, 2)

    def _check(self, rc: int) -> int:
        if rc != OK:
            raise GolHipError(rc, self._L.golhip_batch_last_error(self._h).decode() or
                              self._L.golhip_strerror(rc).decode())
        return rc

    def close(self):
        if self._h:
            self._L.golhip_batch_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):  # pragma: no cover
        try:
            self.close()
        except Exception:
            pass

    def load(self, boards: np.ndarray, first: int = 0):
        """Boards [first, first + n) from an (n, h, w) array of 0 / nonzero bytes (any strides whose
        cells are contiguous within a row).  Resets the turn and the settle records."""
        boards = np.asarray(boards, dtype=np.uint8)
        assert boards.ndim == 3 and boards.shape[1:] == (self.height, self.width), boards.shape
        if boards.strides[2] != 1 or boards.strides[1] < self.width or boards.strides[0] < 0:
            boards = np.ascontiguousarray(boards)
        self._check(self._L.golhip_batch_load_bytes(self._h, first, boards.shape[0], boards.ctypes.data,
                                                    boards.strides[1], boards.strides[0]))

    def init_random(self, seeds=None, seed0: int = 0, density_q32: int = DENSITY_HALF):
        """Board i as Engine.init_random(seed_i, density_q32) of a single engine of this size,
        seed_i = seeds[i] if seeds is given, else seed0 + i; with a soup_box set, every cell outside
        the box cleared."""
        ptr = None
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
            assert seeds.shape == (self.nboards,), seeds.shape
            ptr = seeds.ctypes.data
        self._check(self._L.golhip_batch_init_random(self._h, ptr, seed0, density_q32))

    def store(self, first: int = 0, n: int | None = None, out: np.ndarray | None = None) -> np.ndarray:
        """Boards [first, first + n) as 0 / 255 bytes, (n, h, w).  out: a uint8 (n, h, w) array (or
        view: rows may be padded) to fill instead of a new one."""
        n = self.nboards - first if n is None else n
        if out is None:
            out = np.empty((max(n, 0), self.height, self.width), dtype=np.uint8)
        assert out.dtype == np.uint8 and out.shape == (n, self.height, self.width) and out.strides[2] == 1
        self._check(self._L.golhip_batch_store_bytes(self._h, first, n, out.ctypes.data, out.strides[1],
                                                     out.strides[0]))
        return out

    def step(self, turns: int, history: bool = False) -> np.ndarray | None:
        """Advance every board `turns` generations.  history: return the (nboards, turns) uint32
        alive counts after each turn of this call."""
        if history:
            out = np.zeros((self.nboards, max(turns, 0)), dtype=np.uint32)
            if turns > 0:
                self._check(self._L.golhip_batch_step(self._h, turns, out.ctypes.data, turns))
            else:
                self._check(self._L.golhip_batch_step(self._h, turns, None, 0))
            return out
        self._check(self._L.golhip_batch_step(self._h, turns, None, 0))
        return None

    def alive_counts(self) -> np.ndarray:
        out = np.zeros(self.nboards, dtype=np.uint32)
        self._check(self._L.golhip_batch_alive_counts(self._h, out.ctypes.data))
        return out

    def track_settle(self, on: bool = True):
        """Settle tracking (golhip_batch_track_settle): enable it after a load, before the first step."""
        self._check(self._L.golhip_batch_track_settle(self._h, int(on)))

    def settled(self) -> np.ndarray:
        """int64 per board: the smallest turn t >= 2 with board(t) == board(t - 2), -1 if not reached."""
        out = np.zeros(self.nboards, dtype=np.int64)
        self._check(self._L.golhip_batch_settled(self._h, out.ctypes.data))
        return out

    def track_period(self, on: bool = True):
        """Period tracking (golhip_batch_track_period): per-board cycle detection on the device, for
        any rule.  Enable it after a load, before the first step; not together with track_settle."""
        self._check(self._L.golhip_batch_track_period(self._h, int(on)))

    def periods(self) -> tuple[np.ndarray, np.ndarray]:
        """(repeat_turn, period), int64 per board.  With s(t) = 2 ** floor(log2 t) - 1, repeat_turn is
        the smallest turn t >= 1 run so far with board(t) == board(s(t)) and period = repeat_turn -
        s(repeat_turn), exactly the period of the cycle the board has entered; both -1 until then.
        An empty board or a still life is (1, 1), a lone blinker (3, 2)."""
        repeat_turn = np.zeros(self.nboards, dtype=np.int64)
        period = np.zeros(self.nboards, dtype=np.int64)
        self._check(self._L.golhip_batch_periods(self._h, repeat_turn.ctypes.data, period.ctypes.data))
        return repeat_turn, period

    def search(self, nsoups: int, *, seeds=None, seed0: int = 0, density_q32: int = DENSITY_HALF, max_turns: int,
               rules=None) -> np.ndarray:
        """A soup search on the device (golhip_batch_search): soup i is the board init_random gives
        seed_i = seeds[i] (seed0 + i without seeds) at density_q32 on this batch's size; one
        workgroup generates it in registers and runs it from generation 0 until it repeats or
        max_turns (1 .. 2 ** 20) have run.  Returns a structured array (SOUP_DTYPE) of nsoups
        records: repeat_turn and period as periods() defines them (-1, -1 without a repeat within
        max_turns), stop_turn = search_stop_turn(repeat_turn, max_turns), the generations the soup
        ran, population, its alive cells then, and reserved = 0.  A record depends on the soup's
        seed, the density, the size, the rule, max_turns, the topology and the soup_box only: the
        soup runs on the batch's topology ("plane": the outside is dead, a glider ends at the border
        instead of circling the board), and with a soup_box set the soup is the seed's board with
        every cell outside the centred box cleared, exactly what init_random then gives.

        The rule is the batch's uniform rule; rules (nsoups rule texts or (birth, survive) pairs,
        checked as set_rules checks its own) gives every soup its own.  nsoups is independent of
        nboards, and the batch's boards, turn, records and tracking switches are left as they were.
        The workflow: search, pick the records of interest, then init_random(seeds=interesting) on
        a batch of that many boards to look at the boards themselves."""
        nsoups = int(nsoups)
        sptr = bptr = vptr = None
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
            if seeds.shape != (max(nsoups, 0),):
                raise GolHipError(ERR_ARG, f"seeds: shape {seeds.shape} for {nsoups} soups")
            sptr = seeds.ctypes.data
        if rules is not None:
            pairs = self._pairs_of(rules, nsoups)
            birth, survive = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
            bptr, vptr = birth.ctypes.data, survive.ctypes.data
        out = np.zeros(max(nsoups, 0), dtype=SOUP_DTYPE)
        self._check(self._L.golhip_batch_search(self._h, nsoups, sptr, seed0, density_q32, max_turns, bptr, vptr,
                                                out.ctypes.data))
        return out

    def search_exact(self, nsoups: int, *, seeds=None, seed0: int = 0, density_q32: int = DENSITY_HALF,
                     max_turns: int, rules=None) -> tuple[np.ndarray, np.ndarray]:
        """search() plus the exact turn at which each soup enters its cycle
        (golhip_batch_search_exact).  Returns (records, cycle_start): records is byte for byte what
        search() returns for the same arguments, cycle_start an int64 array with, for a soup that
        repeated within max_turns, the least t >= 0 with board(t + period) == board(t) -- the soup's
        lifespan, where repeat_turn is only the turn at which Brent's snapshots noticed the cycle,
        always 2 ** j - 1 + period -- and -1 for a soup without a repeat.  0 <= cycle_start <=
        repeat_turn - period, and 0 exactly when the soup itself is on its cycle.  The arguments, the
        rule, the topology, the soup_box and the errors are search()'s; cycle_start depends on what
        a record depends on and nothing else.  A second pass on the device (gol_batch_cycle) re-runs
        each soup from its seed: about cycle_start_floor(repeat_turn, period) + period +
        2 * (cycle_start - floor) generations on top of the search's."""
        nsoups = int(nsoups)
        sptr = bptr = vptr = None
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
            if seeds.shape != (max(nsoups, 0),):
                raise GolHipError(ERR_ARG, f"seeds: shape {seeds.shape} for {nsoups} soups")
            sptr = seeds.ctypes.data
        if rules is not None:
            pairs = self._pairs_of(rules, nsoups)
            birth, survive = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
            bptr, vptr = birth.ctypes.data, survive.ctypes.data
        out = np.zeros(max(nsoups, 0), dtype=SOUP_DTYPE)
        cycle_start = np.zeros(max(nsoups, 0), dtype=np.int64)
        self._check(self._L.golhip_batch_search_exact(self._h, nsoups, sptr, seed0, density_q32, max_turns, bptr,
                                                      vptr, out.ctypes.data, cycle_start.ctypes.data))
        return out, cycle_start

    @staticmethod
    def _pattern_table(patterns):
        """(npat, the ctypes array of Patterns) of census()'s `patterns`; a bad array raises
        GolHipError(ERR_ARG) naming its index."""
        pats = []
        for i, p in enumerate(patterns):
            if isinstance(p, Pattern):
                pats.append(p)
                continue
            try:
                pats.append(pattern(p))
            except GolHipError as e:
                raise GolHipError(e.code, f"pattern {i}: " + str(e).split(": ", 2)[2])
        return len(pats), (Pattern * max(len(pats), 1))(*pats)

    def search_census(self, nsoups: int, patterns, *, seeds=None, seed0: int = 0, density_q32: int = DENSITY_HALF,
                      max_turns: int, rules=None, counts: bool = True, residue: bool = True,
                      ash: bool = False) -> SearchCensus:
        """search_exact() plus the census of each soup's ash, in one call and without boards
        (golhip_batch_search_census).  Returns SearchCensus(records, cycle_start, ash_turn, counts,
        residue, ash): records and cycle_start are search_exact()'s, byte for byte; ash_turn (int64)
        is the turn of the board that was censused, cycle_start <= ash_turn <= repeat_turn, a board on
        the soup's cycle (0 and the seeded board when repeat_turn == period); counts (nsoups, npat)
        uint32 and residue (nsoups,) uint32 are census()'s of that board on the batch's topology; ash
        (nsoups, h, w) uint8 is the board itself, 0 / 1.  An output switched off (counts=False,
        residue=False; ash is off by default) is None and its work is skipped; at least one of the
        three must be on, and without patterns counts must be off.  A soup without a repeat within
        max_turns has ash_turn -1, a counts row of zeros, a dead ash and residue = its record's
        population.

        The recipe that reproduces the censused board of a soup: a Batch of this size with the same
        soup_box and topology (and the soup's rule), init_random(seeds=[seed]), step(ash_turn);
        census() there gives the same row.  The board is not aligned to cycle_start's phase: an
        oscillating ash is seen in the phase of turn ash_turn, so list oscillators in every phase
        (common_objects() does).  ash_turn depends on the record and cycle_start only, and every
        output on what a record depends on plus the patterns: not on nsoups, the position or which
        outputs are on.

        patterns, the errors of a bad pattern and their wording are census()'s; seeds, seed0,
        density_q32, max_turns, rules and their errors are search()'s.  The batch's boards, turn,
        rules, records and switches are left as they were."""
        nsoups = int(nsoups)
        npat, table = self._pattern_table(patterns)
        sptr = bptr = vptr = None
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
            if seeds.shape != (max(nsoups, 0),):
                raise GolHipError(ERR_ARG, f"seeds: shape {seeds.shape} for {nsoups} soups")
            sptr = seeds.ctypes.data
        if rules is not None:
            pairs = self._pairs_of(rules, nsoups)
            birth, survive = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
            bptr, vptr = birth.ctypes.data, survive.ctypes.data
        n = max(nsoups, 0)
        out = np.zeros(n, dtype=SOUP_DTYPE)
        cycle_start = np.zeros(n, dtype=np.int64)
        ash_turn = np.zeros(n, dtype=np.int64)
        c = np.zeros((n, npat), dtype=np.uint32) if counts else None
        r = np.zeros(n, dtype=np.uint32) if residue else None
        a = np.zeros((n, self.height, self.width), dtype=np.uint8) if ash else None
        self._check(self._L.golhip_batch_search_census(
            self._h, nsoups, sptr, seed0, density_q32, max_turns, bptr, vptr, ctypes.addressof(table) if npat else None,
            npat, out.ctypes.data, cycle_start.ctypes.data, ash_turn.ctypes.data, c.ctypes.data if counts else None,
            r.ctypes.data if residue else None, a.ctypes.data if ash else None))
        return SearchCensus(out, cycle_start, ash_turn, c, r, a)

    def census(self, patterns, *, counts: bool = True, residue: bool = True):
        """What the boards hold, by pattern matching on the device (golhip_batch_census).  patterns is
        a sequence of 2-D arrays (1 alive, 0 dead, -1 not looked at: pattern()) or Patterns, at most
        256, e.g. the arrays of common_objects().  Returns (counts, residue): counts (nboards, npat)
        uint32, residue (nboards,) uint32; with counts=False or residue=False that output is None and
        its work is skipped (not both).

        Cells: cell_i(x, y) is board i's cell; on a torus the coordinates are taken mod width and mod
        height, on a plane a cell outside the rectangle is dead.  Match: pattern p matches board i at
        anchor (x, y) when cell_i(x + c, y + r) == alive_p(r, c) for every (r, c) that p looks at.
        Anchors: 0 <= x < width, 0 <= y < height on a torus; -(w - 1) <= x <= width - 1 and
        -(h - 1) <= y <= height - 1 on a plane, so an object at the border, its dead ring outside,
        is counted.  counts[i, p] is the number of matching anchors; overlapping matches each count.
        residue[i] is the number of live cells of board i that no match covers, a match covering the
        cells under its pattern's live cells: 0 means the list explains the whole board.  Without
        patterns residue is alive_counts().  The result for board i depends on board i, the topology
        and the patterns only, counts[:, p] on pattern p only, residue not on the patterns' order.
        Nothing else moves: the boards, the turn, the rules, the records and the switches stay.

        The workflow: (1) search() or search_exact(); (2) pick the seeds of interest; (3)
        Batch(w, h, len(seeds)), init_random(seeds=seeds), step(the largest stop_turn); (4)
        census(...).  An oscillating ash is seen in the phase of the turn the batch is at, which is
        why common_objects() lists oscillators in every phase.  For the ash of the soups of a search
        search_census() does all four in one call, without boards and without the extra generations.

        A bad pattern raises GolHipError(ERR_ARG) naming its index: an array before any device work,
        a Pattern (and a pattern larger than the board, or more than 256) from the library."""
        npat, table = self._pattern_table(patterns)
        c = np.zeros((self.nboards, npat), dtype=np.uint32) if counts else None
        r = np.zeros(self.nboards, dtype=np.uint32) if residue else None
        self._check(self._L.golhip_batch_census(self._h, ctypes.addressof(table) if npat else None, npat,
                                                c.ctypes.data if counts else None,
                                                r.ctypes.data if residue else None))
        return c, r

    def objects(self, max_objects: int = 64, reach: int = 2):
        """Every cluster of live cells of every board, found and hashed on the device
        (golhip_batch_objects).  Returns (nobjects, objects): nobjects (nboards,) int32 is each board's
        number of clusters, all of them; objects (nboards, max_objects) of OBJECT_DTYPE holds the first
        min(nobjects[i], max_objects) of board i in row-major order of their first cell, the rest
        zeros.  max_objects is 1..4096, reach 1 or 2.

        Two live cells are linked when their Chebyshev distance is at most reach (mod width and mod
        height on a torus, in the rectangle on a plane); a cluster is a connected component.  reach
        1 gives 8-connected islands, reach 2 (the default) joins cells whose neighbourhoods share a
        cell, so two clusters cannot influence each other in the next generation.  x, y, w, h are the
        extent (on a torus it starts behind the cluster's run of empty columns; a cluster without
        one winds: x 0, w width, OBJECT_WINDS_X), population the cells, flags OBJECT_WINDS_X / _WINDS_Y /
        _AT_BORDER (a plane only: a cell in the outermost row or column).  hash is the same for every
        translation, rotation and reflection of a cluster that does not wind: object_hash(array) is
        the key of a known object, common_object_hashes() names the commonest.  The tally of a batch:
        np.unique(objects["hash"][np.arange(max_objects) < nobjects[:, None]], return_counts=True).

        The result for a board depends on that board, the topology and reach only; max_objects only
        cuts the list.  Nothing else moves: the boards, the turn, the rules, the records and the
        switches stay."""
        n = np.zeros(self.nboards, dtype=np.int32)
        o = np.zeros((self.nboards, max(int(max_objects), 0)), dtype=OBJECT_DTYPE)
        self._check(self._L.golhip_batch_objects(self._h, int(max_objects), int(reach), n.ctypes.data,
                                                 o.ctypes.data if o.size else None))
        return n, o

    def search_objects(self, nsoups: int, *, max_objects: int = 64, reach: int = 2, seeds=None, seed0: int = 0,
                       density_q32: int = DENSITY_HALF, max_turns: int, rules=None) -> SearchObjects:
        """search_census() with the objects of each soup's ash in the census's place
        (golhip_batch_search_objects).  Returns SearchObjects(records, cycle_start, ash_turn, nobjects,
        objects): the first three are search_census()'s, byte for byte; nobjects (nsoups,) int32 and
        objects (nsoups, max_objects) of OBJECT_DTYPE are objects()'s of the board the recipe of
        search_census() reproduces: init_random(seeds=[seed]), step(ash_turn).  A soup without a repeat
        within max_turns has ash_turn -1 and nobjects 0.  seeds, seed0, density_q32, max_turns, rules
        and their errors are search()'s, max_objects and reach objects()'s.  The batch's boards, turn,
        rules, records and switches are left as they were."""
        nsoups = int(nsoups)
        sptr = bptr = vptr = None
        if seeds is not None:
            seeds = np.ascontiguousarray(seeds, dtype=np.uint64)
            if seeds.shape != (max(nsoups, 0),):
                raise GolHipError(ERR_ARG, f"seeds: shape {seeds.shape} for {nsoups} soups")
            sptr = seeds.ctypes.data
        if rules is not None:
            pairs = self._pairs_of(rules, nsoups)
            birth, survive = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
            bptr, vptr = birth.ctypes.data, survive.ctypes.data
        n = max(nsoups, 0)
        out = np.zeros(n, dtype=SOUP_DTYPE)
        cycle_start = np.zeros(n, dtype=np.int64)
        ash_turn = np.zeros(n, dtype=np.int64)
        nobj = np.zeros(n, dtype=np.int32)
        obj = np.zeros((n, max(int(max_objects), 0)), dtype=OBJECT_DTYPE)
        self._check(self._L.golhip_batch_search_objects(
            self._h, nsoups, sptr, seed0, density_q32, max_turns, bptr, vptr, int(max_objects), int(reach),
            out.ctypes.data, cycle_start.ctypes.data, ash_turn.ctypes.data, nobj.ctypes.data,
            obj.ctypes.data if obj.size else None))
        return SearchObjects(out, cycle_start, ash_turn, nobj, obj)

    @property
    def turn(self) -> int:
        v = ctypes.c_int64()
        self._check(self._L.golhip_batch_turn(self._h, ctypes.byref(v)))
        return v.value

    # -- topology and the soup box
    def set_topology(self, topology: str | int):
        """"torus" or "plane" (golhip_batch_set_topology).  On a plane every neighbour outside the
        width x height rectangle is dead.  Keeps the boards, the turn, the rules and the switches;
        with settle or period tracking on, only at turn 0.  On a plane kernel_form is 0 for B3/S23, 2
        for every other uniform rule, 3 for per-board rules."""
        self._check(self._L.golhip_batch_set_topology(self._h, self._topology_of(topology)))

    @property
    def topology(self) -> str:
        """"torus" or "plane"."""
        v = ctypes.c_int32()
        self._check(self._L.golhip_batch_get_topology(self._h, ctypes.byref(v)))
        return "plane" if v.value == TOPOLOGY_PLANE else "torus"

    def set_soup_box(self, box: tuple[int, int] | None):
        """(w, h) with 1 <= w <= width and 1 <= h <= height, or None / (0, 0) for the whole board
        (golhip_batch_set_soup_box).  The box sits at ((width - w) // 2, (height - h) // 2);
        init_random and search clear every cell of a soup outside it, load ignores it."""
        w, h = (0, 0) if box is None else (int(v) for v in box)
        self._check(self._L.golhip_batch_set_soup_box(self._h, w, h))

    @property
    def soup_box(self) -> tuple[int, int] | None:
        """The soup box (w, h), None for the whole board."""
        w, h = ctypes.c_int32(), ctypes.c_int32()
        self._check(self._L.golhip_batch_get_soup_box(self._h, ctypes.byref(w), ctypes.byref(h)))
        return None if (w.value, h.value) == (0, 0) else (w.value, h.value)

    # -- the rule
    def set_rule(self, rule: str | tuple[int, int]):
        """One rule for all boards (golhip_batch_set_rule): "B36/S23" or (birth, survive) masks.  Keeps
        the boards, the turn and the tracking switches; with settle or period tracking on, only at
        turn 0."""
        if isinstance(rule, (str, bytes)):
            self._check(self._L.golhip_batch_set_rule(self._h, rule.encode() if isinstance(rule, str) else rule))
        else:
            birth, survive = self._masks_of(rule)
            self._check(self._L.golhip_batch_set_rule_masks(self._h, birth, survive))

    def set_rules(self, rules):
        """One rule per board (golhip_batch_set_rules): a sequence of nboards rule texts or (birth,
        survive) pairs, or an (nboards, 2) integer array; None: back to the uniform rule.  Per-board
        rules always run the table form of the kernel (kernel_form == 3)."""
        if rules is None:
            self._check(self._L.golhip_batch_set_rules(self._h, None, None))
            return
        pairs = self._pairs_of(rules, self.nboards)
        birth, survive = np.ascontiguousarray(pairs[:, 0]), np.ascontiguousarray(pairs[:, 1])
        self._check(self._L.golhip_batch_set_rules(self._h, birth.ctypes.data, survive.ctypes.data))

    @property
    def rule_masks(self) -> tuple[int, int]:
        """The uniform rule's (birth, survive); GolHipError(ERR_STATE) while per-board rules are set."""
        b, s = ctypes.c_uint32(), ctypes.c_uint32()
        self._check(self._L.golhip_batch_get_rule(self._h, ctypes.byref(b), ctypes.byref(s)))
        return b.value, s.value

    @property
    def rule(self) -> str:
        """The uniform rule in canonical form, e.g. "B36/S23"."""
        return rule_string(*self.rule_masks)

    @property
    def rules(self) -> np.ndarray:
        """(nboards, 2) uint32: every board's (birth, survive), the uniform rule repeated when no
        per-board rules are set."""
        birth, survive = np.zeros(self.nboards, dtype=np.uint32), np.zeros(self.nboards, dtype=np.uint32)
        self._check(self._L.golhip_batch_get_rules(self._h, birth.ctypes.data, survive.ctypes.data))
        return np.stack([birth, survive], axis=1)

    @property
    def kernel_form(self) -> int:
        """What the next step launches: 0 gol_batch (B3/S23), 1 gol_batch_rule constant-folded, 2 its
        table form, 3 the table form with per-board rules.  On a plane: 0, 2 or 3 (no constant-folded
        kernels there)."""
        v = ctypes.c_int32()
        self._check(self._L.golhip_batch_kernel(self._h, ctypes.byref(v)))
        return v.value
