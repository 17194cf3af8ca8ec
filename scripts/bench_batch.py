#!/usr/bin/env python3
"""Cell updates per second of golhip.Batch (many small tori, one gol_batch launch) on the GPU.

For 64 x 64, 128 x 64 and 512 x 512 boards and B in {1, 256, 4096, 65536} boards per batch (where
the boards and their settle copy fit in 16 GiB), calls of 1000 turns in three modes:

  plain          Batch.step(1000)
  history        Batch.step(1000, history=True): every board's alive count after every turn, in a
                 fresh (B, 1000) uint32 host array per call
  history+settle the same with Batch.track_settle() on; its cost is reported as the ratio of its
                 call time to the history mode's

Every figure is a host clock around a whole call, which ends in a device synchronise: 2 warm calls,
then --calls (>= 7) timed ones, the median; rate = B * width * height * 1000 / median.

The yardstick is the only route there was before the batch, measured in the same process: ONE
Engine of that size with set_board_kernel(1), and per board load() + step(1000) + store() (with
counts=True beside the history modes), timed over --yardstick-boards boards; a batch of B boards is
set beside B times its median.  --ceiling-json: the JSON line of a bench.py run of the same
session (its "value", GCUPS at 65536^2), quoted beside the rates.

--rule RULE ("B36/S23", ...): the batch runs that life-like rule (gol_batch_rule: constant-folded for
a catalogue rule, else the table form; with --per-board-rules the same rule given to every board as
its own, which always runs the table form).  The yardstick is then the only route there was for
such a rule: one Engine with set_rule(RULE), per board load() + step(1000) + store().  Every row
also times the B3/S23 batch (gol_batch) of the same size and mode in the same process and reports
the rule's call time over it ("vs_life").  --shapes / --batches narrow the run.  Without --rule the
run and its output are what they always were.

--period: the cost of period tracking (Batch.track_period, gol_batch_period) instead of the run
above.  For every shape and B, plain and with history, the same process times the untracked call,
the call with period tracking on and the call with settle tracking on (all under --rule, B3/S23
without it) and reports period_ratio and settle_ratio: tracked call time over untracked.  The model
for both is 3 more VALU per word per generation.  No engine yardstick in this leg.

--search: the soup search (Batch.search, gol_batch_search) against the only route there was before
it, instead of the run above.  The same soups (seeds 0 .. --soups - 1 at density 1/2), rule and
max_turns on both routes: (a) Batch(w, h, 4096) and per 4096 soups init_random(seeds), track_period,
step(max_turns), periods(); (b) one Batch.search call.  The records (repeat_turn, period) must agree
before anything is timed.  Reported: soups per second of both, their ratio, the mean stop_turn of
the search and the soups that repeated.  The cases: 64 x 64 and 512 x 512 under B3/S23, 64 x 64 under
HighLife and under B38/S0236 (where no soup repeats); max_turns 16384 at 64 x 64, 4096 at 512 x 512.

--plane: the bounded plane (Batch(topology="plane"): gol_plane_rule / _period / _search) beside the
torus, instead of the run above: --search's soups, rules and method, both topologies in this
process.  Per case and topology: the step route over the first 4096 soups (init_random(seeds),
track_period, step(max_turns), periods()) and one Batch.search call of --soups soups; the plane's
search records (repeat_turn, period) of the first 4096 soups must equal the plane step route's
before anything is timed.  Reported: call times, soups per second and plane / torus ratios of both
routes.  The cases: 64 x 64 and 512 x 512 under B3/S23 and under B38/S0236 (the table form);
--max-turns overrides their max_turns.  --box WxH adds the soup box to every batch of this leg
(the boxed search: the share of soups that repeated, their mean repeat_turn, soups per second).

--exact: the exact search (Batch.search_exact: the search plus gol_batch_cycle, which gives every
soup's cycle_start) beside the plain search, instead of the run above: one search_exact call and
one search call on the same --soups soups (seeds 0 .. --soups - 1, any count), 64 x 64 under B3/S23
and under HighLife (whose exact pass runs the table form) at max_turns 16384.  Before anything is
timed the records must agree byte for byte and cycle_start must lie between cycle_start_floor and
repeat_turn - period.  Reported: both call times and their ratio, mean cycle_start beside mean
repeat_turn, and the generations the pass adds (floor + period + 2 (cycle_start - floor), summed
over the soups that repeated) over the sum of repeat_turn and over the sum of stop_turn, the
generations the search itself ran: the ratio the time ratio should track.

--census: the census (Batch.census, gol_batch_census) instead of the run above.  --batches boards (4096
and 65536 by default) of 64 x 64, seeds 0 .. B - 1 at density 1/2, stepped 2000 turns on the torus, and
the 33 arrays of common_objects().  Before anything is timed counts and residue must equal a numpy
brute force of the definitions on the first 64 boards.  Timed: (a) the only route there was,
store() of every board, alone, and with the brute force's time on the 64-board sample scaled to B
boards added; (b) one census call, with the residue and without.  One search call on the same seeds
and the 2000-turn step are timed once each, for scale.

--search-census: Batch.search_census (the exact search with a census of each soup's ash, no boards kept)
instead of the run above.  --batches soups (4096 and 65536 by default) of 64 x 64, seeds 0 .. B - 1 at
density 1/2 under B3/S23, max_turns 16384 (--max-turns), the 33 arrays of common_objects().  Before
anything is timed the records and cycle_start must be search_exact's, cycle_start <= ash_turn <=
repeat_turn must hold, ash_turn must be search_census_turn's, and for 8 soups init_random(seed) +
step(ash_turn) + census on a one-board batch must reproduce the row.  Timed, host clock around whole
calls: (a) search_exact of this library alternated call by call with search_exact of --parent-lib (a
build of the commit before this call existed), with the parent's own min and max as the run-to-run
spread; (b) search_census beside search_exact; (c) the route it replaces, search_exact + init_random
+ step(the largest stop_turn) + census on a batch of B boards (--route-calls times: a call steps every
board to the slowest soup's turn).  Also the ash totals per object.

--objects: the objects (Batch.objects, Batch.search_objects; gol_batch_objects) instead of the run above.
--batches boards (4096 and 65536 by default) of 64 x 64, seeds 0 .. B - 1 at density 1/2, stepped 2000
turns on the torus under B3/S23, reach 2, max_objects 64.  Before anything is timed nobjects and the
records must equal np_objects (tests/objects_cases.py) on the first 256 boards.  Timed, host clock around
whole calls: (a) the route it replaces, store() of every board, alone, and with np_objects' time on
the 256-board sample scaled to B boards added; (b) one objects call, and the counts alone; (c) one
census call with the 33 arrays of common_objects() on the same boards; (d) search_objects beside
search_census on the same seeds (max_turns 16384, --max-turns).  Also the tally of the ashes: np.unique
over the hashes, named where common_object_hashes() knows the hash.

One JSON line on stdout; --out also writes it to a file.  There is no CPU fallback: without a GPU
the script fails.
"""
import argparse
import json
import statistics
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parents[1]
sys.path.insert(0, str(ROOT / "distributed-gol_amd"))
import golhip  # noqa: E402

TURNS = 1000
SHAPES = [(64, 64), (128, 64), (512, 512)]
BATCHES = [1, 256, 4096, 65536]


def median_s(fn, warm, calls):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), min(ts)


def period_leg(a, shapes, batches, rule, res):
    """Untracked, period-tracked and settle-tracked calls of the same size, rule and mode, side by
    side in this process."""
    res["bench"] = "batch_period"
    for w, h in shapes:
        entry = {"width": w, "height": h, "batches": []}
        for B in batches:
            row = {"boards": B}
            for mode in ("plain", "history"):
                hist = mode == "history"
                ms = {}
                for track in ("none", "period", "settle"):
                    with golhip.Batch(w, h, B) as b:
                        b.init_random(seed0=1)
                        if rule and a.per_board_rules:
                            b.set_rules(np.tile(np.array(rule, dtype=np.uint32), (B, 1)))
                        elif rule:
                            b.set_rule(rule)
                        if track == "period":
                            b.track_period()
                        elif track == "settle":
                            b.track_settle()
                        form = b.kernel_form
                        med, best = median_s(lambda: b.step(TURNS, history=hist), 2, a.calls)
                        if track == "period":
                            repeats = int(np.count_nonzero(b.periods()[0] > 0))
                    ms[track] = (med, best)
                row[mode] = {"kernel_form": form, "boards_with_a_repeat": repeats,
                             "call_ms_median": round(ms["none"][0] * 1e3, 3),
                             "call_ms_min": round(ms["none"][1] * 1e3, 3),
                             "period_call_ms_median": round(ms["period"][0] * 1e3, 3),
                             "period_call_ms_min": round(ms["period"][1] * 1e3, 3),
                             "settle_call_ms_median": round(ms["settle"][0] * 1e3, 3),
                             "settle_call_ms_min": round(ms["settle"][1] * 1e3, 3),
                             "gcups": round(B * w * h * TURNS / ms["none"][0] / 1e9, 2),
                             "period_gcups": round(B * w * h * TURNS / ms["period"][0] / 1e9, 2),
                             "period_ratio": round(ms["period"][0] / ms["none"][0], 3),
                             "settle_ratio": round(ms["settle"][0] / ms["none"][0], 3)}
            entry["batches"].append(row)
            print(json.dumps({"shape": [w, h], **row}), file=sys.stderr, flush=True)
        res["shapes"].append(entry)


SEARCH_CASES = [(64, 64, "B3/S23", 16384), (512, 512, "B3/S23", 4096), (64, 64, "B36/S23", 16384),
                (64, 64, "B38/S0236", 16384)]
SEARCH_BATCH = 4096


def search_leg(a, res):
    """The step route and the search on the same soups, rule and max_turns, side by side in this
    process."""
    res["bench"] = "batch_search"
    res["soups"] = a.soups
    del res["turns"]
    assert a.soups >= 1 and a.soups % SEARCH_BATCH == 0, "--soups: a multiple of 4096"
    seeds = np.arange(a.soups, dtype=np.uint64)
    for w, h, rule, max_turns in SEARCH_CASES:
        if a.shapes and (w, h) not in [tuple(int(v) for v in t.split("x")) for t in a.shapes.split(",")]:
            continue
        with golhip.Batch(w, h, SEARCH_BATCH, rule=rule) as b:
            form = b.kernel_form

            def step_route():
                turns, periods = [], []
                for i in range(0, a.soups, SEARCH_BATCH):
                    b.init_random(seeds=seeds[i:i + SEARCH_BATCH])
                    b.track_period()
                    b.step(max_turns)
                    t, p = b.periods()
                    turns.append(t)
                    periods.append(p)
                return np.concatenate(turns), np.concatenate(periods)

            def search():
                return b.search(a.soups, seeds=seeds, max_turns=max_turns)

            turns, periods = step_route()
            got = search()
            assert np.array_equal(got["repeat_turn"], turns) and np.array_equal(got["period"], periods), (w, h, rule)
            step_med, step_min = median_s(step_route, 2, a.calls)
            search_med, search_min = median_s(search, 2, a.calls)
        row = {"width": w, "height": h, "rule": rule, "kernel_form": form, "max_turns": max_turns,
               "soups_with_a_repeat": int(np.count_nonzero(turns > 0)),
               "mean_repeat_turn": round(float(turns[turns > 0].mean()), 1) if (turns > 0).any() else None,
               "mean_stop_turn": round(float(got["stop_turn"].mean()), 1),
               "step_route_ms_median": round(step_med * 1e3, 3), "step_route_ms_min": round(step_min * 1e3, 3),
               "search_ms_median": round(search_med * 1e3, 3), "search_ms_min": round(search_min * 1e3, 3),
               "step_route_soups_per_s": round(a.soups / step_med, 1),
               "search_soups_per_s": round(a.soups / search_med, 1),
               "search_over_step_route": round(step_med / search_med, 3)}
        res["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)


PLANE_CASES = [(64, 64, "B3/S23", 16384), (512, 512, "B3/S23", 4096), (64, 64, "B38/S0236", 16384),
               (512, 512, "B38/S0236", 4096)]


def plane_leg(a, res):
    """Torus and plane on the same soups, rule and max_turns, side by side in this process: the step
    route over 4096 boards and the search over --soups soups."""
    res["bench"] = "batch_plane"
    res["soups"] = a.soups
    del res["turns"]
    assert a.soups >= 1 and a.soups % SEARCH_BATCH == 0, "--soups: a multiple of 4096"
    box = tuple(int(v) for v in a.box.split("x")) if a.box else None
    res["soup_box"] = box
    seeds = np.arange(a.soups, dtype=np.uint64)
    rules = [golhip.rule_string(*golhip.parse_rule(r)) for r in a.rule.split(",")] if a.rule else None
    for w, h, rule, max_turns in PLANE_CASES:
        if a.shapes and (w, h) not in [tuple(int(v) for v in t.split("x")) for t in a.shapes.split(",")]:
            continue
        if rules and golhip.rule_string(*golhip.parse_rule(rule)) not in rules:
            continue
        max_turns = a.max_turns or max_turns
        row = {"width": w, "height": h, "rule": rule, "max_turns": max_turns}
        for topology in ("torus", "plane"):
            with golhip.Batch(w, h, SEARCH_BATCH, rule=rule, topology=topology, soup_box=box) as b:

                def step_route():
                    b.init_random(seeds=seeds[:SEARCH_BATCH])
                    b.track_period()
                    b.step(max_turns)
                    return b.periods()

                def search():
                    return b.search(a.soups, seeds=seeds, max_turns=max_turns)

                turns, periods = step_route()
                got = search()
                head = got[:SEARCH_BATCH]
                assert np.array_equal(head["repeat_turn"], turns) and np.array_equal(head["period"], periods), \
                    (w, h, rule, topology)
                step_med, step_min = median_s(step_route, 2, a.calls)
                search_med, search_min = median_s(search, 2, a.calls)
                rt = got["repeat_turn"]
                row[topology] = {
                    "kernel_form": b.kernel_form,
                    "step_route_ms_median": round(step_med * 1e3, 3), "step_route_ms_min": round(step_min * 1e3, 3),
                    "step_route_gcups": round(SEARCH_BATCH * w * h * max_turns / step_med / 1e9, 1),
                    "search_ms_median": round(search_med * 1e3, 3), "search_ms_min": round(search_min * 1e3, 3),
                    "search_soups_per_s": round(a.soups / search_med, 1),
                    "share_repeated": round(float((rt > 0).mean()), 4),
                    "mean_repeat_turn": round(float(rt[rt > 0].mean()), 1) if (rt > 0).any() else None,
                    "max_period": int(got["period"].max()),
                    "mean_stop_turn": round(float(got["stop_turn"].mean()), 1)}
        row["plane_over_torus_step_route"] = round(row["plane"]["step_route_ms_median"] /
                                                   row["torus"]["step_route_ms_median"], 3)
        row["plane_over_torus_search"] = round(row["plane"]["search_ms_median"] / row["torus"]["search_ms_median"], 3)
        res["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)


EXACT_CASES = [(64, 64, "B3/S23", 16384), (64, 64, "B36/S23", 16384)]


def exact_leg(a, res):
    """Batch.search_exact beside Batch.search on the same soups, rule and max_turns, in this process."""
    res["bench"] = "batch_cycle"
    res["soups"] = a.soups
    del res["turns"]
    assert a.soups >= 1
    seeds = np.arange(a.soups, dtype=np.uint64)
    for w, h, rule, max_turns in EXACT_CASES:
        max_turns = a.max_turns or max_turns
        with golhip.Batch(w, h, 1, rule=rule) as b:
            form = b.kernel_form

            def search():
                return b.search(a.soups, seeds=seeds, max_turns=max_turns)

            def exact():
                return b.search_exact(a.soups, seeds=seeds, max_turns=max_turns)

            rec = search()
            got, start = exact()
            assert got.tobytes() == rec.tobytes(), (w, h, rule)
            rep, per = rec["repeat_turn"], rec["period"]
            found = rep > 0
            assert (start[~found] == -1).all() and (start[found] >= 0).all(), (w, h, rule)
            assert (start[found] <= (rep - per)[found]).all(), (w, h, rule)
            lo = np.array([golhip.cycle_start_floor(int(r), int(p)) for r, p in zip(rep, per)], dtype=np.int64)
            assert (lo[found] <= start[found]).all(), (w, h, rule)
            search_med, search_min = median_s(search, 2, a.calls)
            exact_med, exact_min = median_s(exact, 2, a.calls)
        extra = (lo + per + 2 * (start - lo))[found]  # the pass's generations, without its detection slack
        row = {"width": w, "height": h, "rule": rule, "search_kernel_form": form, "max_turns": max_turns,
               "soups_with_a_repeat": int(found.sum()),
               "mean_repeat_turn": round(float(rep[found].mean()), 1) if found.any() else None,
               "mean_cycle_start": round(float(start[found].mean()), 1) if found.any() else None,
               "max_cycle_start": int(start.max()),
               "mean_stop_turn": round(float(rec["stop_turn"].mean()), 1),
               "cycle_start_below_snapshot_turn": int((start < rep - per)[found].sum()),
               "generations_ratio_over_repeat_turn": round(float(extra.sum() / rep[found].sum()), 4) if found.any() else None,
               "generations_ratio_over_stop_turn": round(float(extra.sum() / rec["stop_turn"].sum()), 4),
               "search_ms_median": round(search_med * 1e3, 3), "search_ms_min": round(search_min * 1e3, 3),
               "exact_ms_median": round(exact_med * 1e3, 3), "exact_ms_min": round(exact_min * 1e3, 3),
               "search_soups_per_s": round(a.soups / search_med, 1), "exact_soups_per_s": round(a.soups / exact_med, 1),
               "exact_over_search": round(exact_med / search_med, 3)}
        res["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)


def census_reference(board, patterns, plane=False):
    """(counts, residue) of one board from the definitions of golhip_batch_census in numpy: the route
    a host has without the call, after store()."""
    a = board != 0
    H, W = a.shape
    big = np.pad(a, 31) if plane else np.tile(a, (1 + -(-31 // H), 1 + -(-31 // W)))
    counts, covered = np.zeros(len(patterns), dtype=np.uint32), np.zeros((H, W), dtype=bool)
    for k, p in enumerate(patterns):
        h, w = p.shape
        ny, nx, oy, ox = (H + h - 1, W + w - 1, 32 - h, 32 - w) if plane else (H, W, 0, 0)
        m = np.ones((ny, nx), dtype=bool)
        for r, c in zip(*np.nonzero(p >= 0)):
            m &= big[oy + r:oy + r + ny, ox + c:ox + c + nx] == (p[r, c] == 1)
        counts[k] = m.sum()
        for y, x in zip(*np.nonzero(m)):
            for r, c in zip(*np.nonzero(p == 1)):
                covered[(y + oy - 31 * plane + r) % H, (x + ox - 31 * plane + c) % W] = True
    return counts, int((a & ~covered).sum())


def census_leg(a, res):
    """Batch.census beside the only route there was before it (store() and matching on the host) and
    beside the search that produced the soups, in this process."""
    res["bench"] = "batch_census"
    res["turns"] = CENSUS_TURNS
    objs = golhip.common_objects()
    pats = [p for v in objs.values() for p in v]
    names = [k for k, v in objs.items() for _ in v]
    res["patterns"] = len(pats)
    sample = 64
    for B in ([int(v) for v in a.batches.split(",")] if a.batches else [4096, 65536]):
        seeds = np.arange(B, dtype=np.uint64)
        with golhip.Batch(64, 64, B) as b:
            t0 = time.perf_counter()
            rec = b.search(B, seeds=seeds, max_turns=CENSUS_TURNS)
            search_s = time.perf_counter() - t0
            b.init_random(seeds=seeds)
            t0 = time.perf_counter()
            b.step(CENSUS_TURNS)
            step_s = time.perf_counter() - t0
            counts, residue = b.census(pats)
            head = b.store(0, sample)
            t0 = time.perf_counter()
            want = [census_reference(board, pats) for board in head]
            ref_s = time.perf_counter() - t0
            assert np.array_equal(counts[:sample], np.array([w[0] for w in want])), B
            assert np.array_equal(residue[:sample], np.array([w[1] for w in want])), B
            assert np.array_equal(b.census(pats, residue=False)[0], counts), B
            out = np.empty((B, 64, 64), dtype=np.uint8)
            store_med, store_min = median_s(lambda: b.store(out=out), 2, a.calls)
            both_med, both_min = median_s(lambda: b.census(pats), 2, a.calls)
            cnt_med, cnt_min = median_s(lambda: b.census(pats, residue=False), 2, a.calls)
        totals = {k: int(sum(int(counts[:, i].sum()) for i, n in enumerate(names) if n == k)) for k in objs}
        host_s = store_med + ref_s * B / sample
        row = {"width": 64, "height": 64, "boards": B, "totals": totals,
               "boards_with_residue_0": int((residue == 0).sum()), "soups_with_a_repeat": int((rec["repeat_turn"] > 0).sum()),
               "store_ms_median": round(store_med * 1e3, 3), "store_ms_min": round(store_min * 1e3, 3),
               "reference_ms_per_board": round(ref_s / sample * 1e3, 3), "host_route_ms_scaled": round(host_s * 1e3, 1),
               "census_ms_median": round(both_med * 1e3, 3), "census_ms_min": round(both_min * 1e3, 3),
               "census_counts_only_ms_median": round(cnt_med * 1e3, 3), "census_counts_only_ms_min": round(cnt_min * 1e3, 3),
               "census_boards_per_s": round(B / both_med, 1), "store_over_census": round(store_med / both_med, 2),
               "host_route_over_census": round(host_s / both_med, 1),
               "search_ms_once": round(search_s * 1e3, 3), "step_ms_once": round(step_s * 1e3, 3),
               "census_over_search": round(both_med / search_s, 4)}
        res["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)


CENSUS_TURNS = 2000


def load_older_library(path):
    """A libgolhip.so built from an earlier commit: it lacks the newest exports, which
    golhip.load_library insists on, so what it has is bound with the current signatures."""
    import ctypes

    old, cur = ctypes.CDLL(str(path)), golhip.load_library()
    for name in golhip.EXPORTS:
        if hasattr(old, name):
            getattr(old, name).argtypes = getattr(cur, name).argtypes
            getattr(old, name).restype = getattr(cur, name).restype
    return old


def search_census_leg(a, res):
    """Batch.search_census beside search_exact (this library's and, alternated, the parent build's) and
    beside the four-call route it replaces, in this process."""
    res["bench"] = "batch_search_census"
    max_turns = a.max_turns or 16384
    res["max_turns"] = max_turns
    objs = golhip.common_objects()
    pats = [p for v in objs.values() for p in v]
    names = [k for k, v in objs.items() for _ in v]
    res["patterns"] = len(pats)
    parent = load_older_library(a.parent_lib) if a.parent_lib else None
    res["parent_version"] = parent.golhip_version() if parent else None
    for B in ([int(v) for v in a.batches.split(",")] if a.batches else [4096, 65536]):
        seeds = np.arange(B, dtype=np.uint64)
        with golhip.Batch(64, 64, 1) as b:
            got = b.search_census(B, pats, seeds=seeds, max_turns=max_turns)
            rec, start = b.search_exact(B, seeds=seeds, max_turns=max_turns)
            assert got.records.tobytes() == rec.tobytes() and np.array_equal(got.cycle_start, start), B
            found = rec["repeat_turn"] > 0
            assert ((start <= got.ash_turn) & (got.ash_turn <= rec["repeat_turn"]))[found].all(), B
            assert (got.ash_turn[~found] == -1).all() and np.array_equal(got.residue[~found], rec["population"][~found])
            model = [golhip.search_census_turn(int(r), int(p), int(s))
                     for r, p, s in zip(rec["repeat_turn"][:4096], rec["period"][:4096], start[:4096])]
            assert got.ash_turn[:4096].tolist() == model, B
            for i in np.nonzero(found)[0][:8]:  # the recipe
                with golhip.Batch(64, 64, 1) as look:
                    look.init_random(seeds=seeds[i:i + 1])
                    look.step(int(got.ash_turn[i]))
                    c1, r1 = look.census(pats)
                assert np.array_equal(c1[0], got.counts[i]) and r1[0] == got.residue[i], (B, i)

            def exact():
                return b.search_exact(B, seeds=seeds, max_turns=max_turns)

            def census():
                return b.search_census(B, pats, seeds=seeds, max_turns=max_turns)

            tree_ts, parent_ts = [], []
            if parent:
                with golhip.Batch(64, 64, 1, lib=parent) as pb:
                    def parent_exact():
                        return pb.search_exact(B, seeds=seeds, max_turns=max_turns)

                    prec, pstart = parent_exact()
                    assert prec.tobytes() == rec.tobytes() and np.array_equal(pstart, start), B
                    for fn in (parent_exact, exact, parent_exact, exact):  # 2 warm calls each
                        fn()
                    for _ in range(a.calls):
                        for fn, ts in ((parent_exact, parent_ts), (exact, tree_ts)):
                            t0 = time.perf_counter()
                            fn()
                            ts.append(time.perf_counter() - t0)
                exact_med, exact_min = statistics.median(tree_ts), min(tree_ts)
            else:
                exact_med, exact_min = median_s(exact, 2, a.calls)
            census_med, census_min = median_s(census, 2, a.calls)
        lib = parent if parent else None
        with golhip.Batch(64, 64, B, lib=lib) as rb:
            def route():
                r, _ = rb.search_exact(B, seeds=seeds, max_turns=max_turns)
                rb.init_random(seeds=seeds)
                rb.step(int(r["stop_turn"].max()))
                return rb.census(pats)

            route_med, route_min = median_s(route, 2, a.route_calls)
        totals = {k: int(sum(int(got.counts[:, i].sum()) for i, n in enumerate(names) if n == k)) for k in objs}
        row = {"width": 64, "height": 64, "soups": B, "totals": totals,
               "soups_with_a_repeat": int(found.sum()), "soups_with_residue_0": int((got.residue == 0).sum()),
               "mean_repeat_turn": round(float(rec["repeat_turn"][found].mean()), 1),
               "mean_ash_turn": round(float(got.ash_turn[found].mean()), 1), "max_stop_turn": int(rec["stop_turn"].max()),
               "exact_ms_median": round(exact_med * 1e3, 3), "exact_ms_min": round(exact_min * 1e3, 3),
               "exact_ms_max": round(max(tree_ts) * 1e3, 3) if tree_ts else None,
               "parent_exact_ms_median": round(statistics.median(parent_ts) * 1e3, 3) if parent_ts else None,
               "parent_exact_ms_min": round(min(parent_ts) * 1e3, 3) if parent_ts else None,
               "parent_exact_ms_max": round(max(parent_ts) * 1e3, 3) if parent_ts else None,
               "exact_over_parent_exact": round(exact_med / statistics.median(parent_ts), 4) if parent_ts else None,
               "search_census_ms_median": round(census_med * 1e3, 3), "search_census_ms_min": round(census_min * 1e3, 3),
               "search_census_over_exact": round(census_med / exact_med, 4),
               "route_calls": a.route_calls, "route_library": "parent" if parent else "this",
               "route_ms_median": round(route_med * 1e3, 1), "route_ms_min": round(route_min * 1e3, 1),
               "route_over_search_census": round(route_med / census_med, 2)}
        res["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)


def objects_leg(a, res):
    """Batch.objects beside the route it replaces (store() and labelling on the host) and beside the
    census, Batch.search_objects beside search_census, in this process."""
    sys.path.insert(0, str(ROOT / "tests"))
    import objects_cases

    res["bench"] = "batch_objects"
    res["turns"] = CENSUS_TURNS
    res["reach"], res["max_objects"] = 2, 64
    pats = [p for v in golhip.common_objects().values() for p in v]
    known = golhip.common_object_hashes()
    max_turns = a.max_turns or 16384
    sample = 256
    for B in ([int(v) for v in a.batches.split(",")] if a.batches else [4096, 65536]):
        seeds = np.arange(B, dtype=np.uint64)
        with golhip.Batch(64, 64, B) as b:
            b.init_random(seeds=seeds)
            b.step(CENSUS_TURNS)
            nobj, obj = b.objects()
            head = b.store(0, min(sample, B))
            t0 = time.perf_counter()
            want = objects_cases.np_objects(head, "torus", 2)
            ref_s = time.perf_counter() - t0
            wn, wo = objects_cases.table(want, 64)
            assert np.array_equal(nobj[:len(head)], wn) and np.array_equal(obj[:len(head)], wo), B
            assert np.array_equal(b.objects(max_objects=1)[0], nobj), B
            out = np.empty((B, 64, 64), dtype=np.uint8)
            store_med, store_min = median_s(lambda: b.store(out=out), 2, a.calls)
            obj_med, obj_min = median_s(lambda: b.objects(), 2, a.calls)
            lib, h = golhip.load_library(), b._h
            cnt_med, cnt_min = median_s(lambda: lib.golhip_batch_objects(h, 64, 2, nobj.ctypes.data, None), 2, a.calls)
            census_med, census_min = median_s(lambda: b.census(pats), 2, a.calls)
            counts, _ = b.census(pats)
        with golhip.Batch(64, 64, 1) as b:
            so_med, so_min = median_s(lambda: b.search_objects(B, seeds=seeds, max_turns=max_turns), 2, a.calls)
            sc_med, sc_min = median_s(lambda: b.search_census(B, pats, seeds=seeds, max_turns=max_turns), 2, a.calls)
            so = b.search_objects(B, seeds=seeds, max_turns=max_turns)
        tally = {}
        for name, got_n, got_o in (("turn_2000", nobj, obj), ("search_ash", so.nobjects, so.objects)):
            listed = got_o["hash"][np.arange(64)[None, :] < np.minimum(got_n, 64)[:, None]]
            hashes, times = np.unique(listed, return_counts=True)
            named = {}
            for hsh, t in zip(hashes.tolist(), times.tolist()):
                named[known.get(hsh, "other")] = named.get(known.get(hsh, "other"), 0) + t
            top = sorted(zip(times.tolist(), hashes.tolist()), reverse=True)[:12]
            tally[name] = {"clusters": int(got_n.sum()), "distinct_hashes": len(hashes), "named": named,
                           "boards_over_the_cap": int((got_n > 64).sum()), "most_clusters": int(got_n.max()),
                           "top": [[f"{hsh:016x}", t, known.get(hsh, "")] for t, hsh in top]}
        host_s = store_med + ref_s * B / len(head)
        row = {"width": 64, "height": 64, "boards": B, "tally": tally,
               "census_match_totals": {k: int(sum(int(counts[:, i].sum()) for i, n in enumerate(
                   [k2 for k2, v in golhip.common_objects().items() for _ in v]) if n == k)) for k in golhip.common_objects()},
               "store_ms_median": round(store_med * 1e3, 3), "store_ms_min": round(store_min * 1e3, 3),
               "reference_ms_per_board": round(ref_s / len(head) * 1e3, 3), "host_route_ms_scaled": round(host_s * 1e3, 1),
               "objects_ms_median": round(obj_med * 1e3, 3), "objects_ms_min": round(obj_min * 1e3, 3),
               "objects_counts_only_ms_median": round(cnt_med * 1e3, 3), "objects_counts_only_ms_min": round(cnt_min * 1e3, 3),
               "census_ms_median": round(census_med * 1e3, 3), "census_ms_min": round(census_min * 1e3, 3),
               "objects_boards_per_s": round(B / obj_med, 1), "store_over_objects": round(store_med / obj_med, 3),
               "host_route_over_objects": round(host_s / obj_med, 1), "objects_over_census": round(obj_med / census_med, 3),
               "max_turns": max_turns,
               "search_objects_ms_median": round(so_med * 1e3, 3), "search_objects_ms_min": round(so_min * 1e3, 3),
               "search_census_ms_median": round(sc_med * 1e3, 3), "search_census_ms_min": round(sc_min * 1e3, 3),
               "search_objects_over_search_census": round(so_med / sc_med, 4)}
        assert obj_med <= host_s, (obj_med, host_s)  # no slower than the route it replaces
        res["shapes"].append(row)
        print(json.dumps(row), file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=7)
    ap.add_argument("--yardstick-boards", type=int, default=32)
    ap.add_argument("--ceiling-json", type=Path)
    ap.add_argument("--out", type=Path)
    ap.add_argument("--rule")
    ap.add_argument("--per-board-rules", action="store_true")
    ap.add_argument("--shapes", help="e.g. 64x64,512x512 (default: all three)")
    ap.add_argument("--batches", help="e.g. 256,4096 (default: 1,256,4096,65536)")
    ap.add_argument("--period", action="store_true", help="the cost of period tracking (see above)")
    ap.add_argument("--search", action="store_true", help="the soup search against the step route (see above)")
    ap.add_argument("--soups", type=int, default=4096, help="--search, --plane: soups per call, a multiple of 4096")
    ap.add_argument("--plane", action="store_true", help="the plane beside the torus (see above)")
    ap.add_argument("--box", help="--plane: the soup box, e.g. 16x16")
    ap.add_argument("--max-turns", type=int, help="--plane, --exact, --objects: instead of the cases' max_turns")
    ap.add_argument("--exact", action="store_true", help="search_exact beside search (see above)")
    ap.add_argument("--census", action="store_true", help="Batch.census beside store() + numpy (see above)")
    ap.add_argument("--search-census", action="store_true",
                    help="Batch.search_census beside search_exact and the route it replaces (see above)")
    ap.add_argument("--objects", action="store_true",
                    help="Batch.objects beside store() + numpy and the census, search_objects beside search_census")
    ap.add_argument("--parent-lib", type=Path, help="--search-census: a libgolhip.so built from the parent commit")
    ap.add_argument("--route-calls", type=int, default=3, help="--search-census: timed calls of the replaced route")
    a = ap.parse_args()
    assert a.calls >= 7
    assert a.rule or not a.per_board_rules, "--per-board-rules needs --rule"
    if a.objects:
        assert not (a.search_census or a.census or a.exact or a.plane or a.search or a.period or a.rule), \
            "--objects replaces the other legs"
        res = {"bench": "batch_objects", "version": golhip.load_library().golhip_version(), "calls": a.calls, "shapes": []}
        objects_leg(a, res)
        line = json.dumps(res)
        print(line)
        if a.out:
            a.out.parent.mkdir(parents=True, exist_ok=True)
            a.out.write_text(line + "\n")
        return
    if a.search_census:
        assert not (a.census or a.exact or a.plane or a.search or a.period or a.rule), "--search-census replaces the other legs"
        res = {"bench": "batch_search_census", "version": golhip.load_library().golhip_version(), "calls": a.calls,
               "shapes": []}
        search_census_leg(a, res)
        line = json.dumps(res)
        print(line)
        if a.out:
            a.out.parent.mkdir(parents=True, exist_ok=True)
            a.out.write_text(line + "\n")
        return
    if a.census:
        assert not (a.exact or a.plane or a.search or a.period or a.rule), "--census replaces the other legs"
        res = {"bench": "batch_census", "version": golhip.load_library().golhip_version(), "turns": None,
               "calls": a.calls, "shapes": []}
        census_leg(a, res)
        line = json.dumps(res)
        print(line)
        if a.out:
            a.out.parent.mkdir(parents=True, exist_ok=True)
            a.out.write_text(line + "\n")
        return
    if a.exact:
        assert not (a.plane or a.search or a.period or a.rule), "--exact has its own rules and replaces the other legs"
        res = {"bench": "batch_cycle", "version": golhip.load_library().golhip_version(), "turns": None,
               "calls": a.calls, "shapes": []}
        exact_leg(a, res)
        line = json.dumps(res)
        print(line)
        if a.out:
            a.out.parent.mkdir(parents=True, exist_ok=True)
            a.out.write_text(line + "\n")
        return
    if a.plane:  # --rule here selects among the leg's cases ("B3/S23,B38/S0236")
        assert not (a.search or a.period or a.per_board_rules), "--plane replaces the other legs"
        res = {"bench": "batch_plane", "version": golhip.load_library().golhip_version(), "turns": None,
               "calls": a.calls, "shapes": []}
        plane_leg(a, res)
        line = json.dumps(res)
        print(line)
        if a.out:
            a.out.parent.mkdir(parents=True, exist_ok=True)
            a.out.write_text(line + "\n")
        return
    shapes = [tuple(int(v) for v in t.split("x")) for t in a.shapes.split(",")] if a.shapes else SHAPES
    batches = [int(v) for v in a.batches.split(",")] if a.batches else BATCHES
    rule = golhip.parse_rule(a.rule) if a.rule else None
    res = {"bench": "batch", "version": golhip.load_library().golhip_version(), "turns": TURNS,
           "calls": a.calls, "shapes": []}
    if a.ceiling_json:
        line = [ln for ln in a.ceiling_json.read_text().splitlines() if ln.startswith("{")][-1]
        res["ceiling_65536sq_gcups"] = json.loads(line)["value"]
    if rule:
        res["rule"] = golhip.rule_string(*rule)
        res["per_board_rules"] = a.per_board_rules
    if a.search:
        assert not (a.rule or a.period), "--search has its own rules and replaces the other legs"
        search_leg(a, res)
        shapes = []  # this leg replaces the run below
    if a.period:
        period_leg(a, shapes, batches if a.batches else [256, 4096], rule, res)
        shapes = []  # this leg replaces the run below
    budget = 16 << 30  # bytes of boards plus their settle copy a batch may take here
    for w, h in shapes:
        cells = w * h
        entry = {"width": w, "height": h, "batches": []}
        # the yardstick: one engine, board after board
        rng = np.random.default_rng(1)
        board = (rng.random((h, w)) < 0.5).astype(np.uint8) * 255
        with golhip.Engine(w, h, k=16) as e:
            if rule:
                e.set_rule(rule)
                assert e.launch_kind(16)[0] == "rule"
            else:
                e.set_board_kernel(1)
                assert e.launch_kind(16)[0] == "board"

            def one(counts):
                e.load(board)
                e.step(TURNS, counts=counts)
                if not counts:
                    e.sync()
                e.store()

            y = {}
            for name, counts in (("plain", False), ("counts", True)):
                med, best = median_s(lambda: one(counts), 3, a.yardstick_boards)
                y[name] = {"per_board_ms_median": round(med * 1e3, 4), "per_board_ms_min": round(best * 1e3, 4),
                           "gcups": round(cells * TURNS / med / 1e9, 3)}
        entry["engine_loop"] = y
        for B in batches:
            words = h * max(w, 128) // 32 * 4  # bytes of one packed board
            if B * words * 2 > budget:
                entry["batches"].append({"boards": B, "skipped": "over 16 GiB of boards"})
                continue
            row = {"boards": B}
            for mode in ("plain", "history", "history+settle"):
                with golhip.Batch(w, h, B) as b:
                    b.init_random(seed0=1)
                    if mode == "history+settle":
                        b.track_settle()
                    hist = mode != "plain"
                    if rule and a.per_board_rules:
                        b.set_rules(np.tile(np.array(rule, dtype=np.uint32), (B, 1)))
                    elif rule:
                        b.set_rule(rule)
                    form = b.kernel_form
                    med, best = median_s(lambda: b.step(TURNS, history=hist), 2, a.calls)
                loop = y["plain" if mode == "plain" else "counts"]["per_board_ms_median"] * 1e-3 * B
                row[mode] = {"call_ms_median": round(med * 1e3, 3), "call_ms_min": round(best * 1e3, 3),
                             "per_board_us": round(med / B * 1e6, 3),
                             "gcups": round(B * cells * TURNS / med / 1e9, 2),
                             "engine_loop_ms": round(loop * 1e3, 3),
                             "speedup_over_engine_loop": round(loop / med, 2)}
                if rule:  # the B3/S23 batch of the same size and mode, same process
                    with golhip.Batch(w, h, B) as b:
                        b.init_random(seed0=1)
                        if mode == "history+settle":
                            b.track_settle()
                        life, _ = median_s(lambda: b.step(TURNS, history=hist), 2, a.calls)
                    row[mode].update(kernel_form=form, life_call_ms_median=round(life * 1e3, 3),
                                     vs_life=round(med / life, 3))
            row["settle_cost_ratio"] = round(row["history+settle"]["call_ms_median"] / row["history"]["call_ms_median"], 3)
            entry["batches"].append(row)
            print(json.dumps({"shape": [w, h], **row}), file=sys.stderr, flush=True)
        res["shapes"].append(entry)
    line = json.dumps(res)
    print(line)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
