#!/usr/bin/env python3
"""Wall-clock timing of golhip_view_counts (the density viewport) on the GPU.

  whole   : a 65536^2 random board (seed 3), the whole board at scale 64 -> 1024^2 counts; the
            kernel streams the packed board once (512 MiB), so the line also gives packed bytes
            read per second of wall time, to set beside bench.py --full's hbm_roofline_k1;
  window  : the same board, a 1024^2 window at scale 1 from an unaligned origin (a latency figure);
  route   : at 16384^2, the only route the engine had before -- store() of the whole board as bytes
            (256 MiB over PCIe) + a numpy block sum at scale 16 -- against view_counts at scale 16
            (32 MiB of HBM read, 4 MiB returned), the two alternating in one run; the results must
            be equal.

Every figure is a host clock around a call that ends in a device synchronise (each call
synchronises the handle and returns the counts in host memory): 3 warm calls, then 20 timed ones
(5 for the store() route: each moves 256 MiB), median and minimum.  One JSON line on stdout; --out
also writes it to a file.  There is no CPU fallback: without a GPU the script fails.
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


def timed(fn, warm=3, calls=20):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return {"calls": calls, "median_ms": round(statistics.median(ts) * 1e3, 3), "min_ms": round(min(ts) * 1e3, 3)}


def block_sum(board, scale):
    h, w = board.shape
    return (board != 0).reshape(h // scale, scale, w // scale, scale).sum(axis=(1, 3), dtype=np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=65536)
    ap.add_argument("--route-size", type=int, default=16384)
    ap.add_argument("--out", type=Path)
    a = ap.parse_args()
    res = {"bench": "view_counts", "version": golhip.load_library().golhip_version()}

    n = a.size
    with golhip.Engine(n, n, k=16) as e:
        e.init_random(3)
        alive = e.alive_count()
        counts = e.view_counts(0, 0, n // 64, n // 64, 64)
        assert int(counts.sum(dtype=np.uint64)) == alive, "view counts do not add up to the alive count"
        t = timed(lambda: e.view_counts(0, 0, n // 64, n // 64, 64))
        packed = n * n // 8
        t.update(board=n, scale=64, pixels=[n // 64, n // 64], packed_bytes_read=packed,
                 read_gbs_median=round(packed / t["median_ms"] / 1e6, 1),
                 read_gbs_best=round(packed / t["min_ms"] / 1e6, 1))
        res["whole"] = t
        # the display loop's form: one page-locked result array reused by every call
        frame = golhip.pinned_empty((n // 64, n // 64), np.uint32)
        t = timed(lambda: e.view_counts(0, 0, n // 64, n // 64, 64, out=frame))
        assert np.array_equal(frame, counts)
        t.update(out="page-locked, reused", read_gbs_median=round(packed / t["median_ms"] / 1e6, 1),
                 read_gbs_best=round(packed / t["min_ms"] / 1e6, 1))
        res["whole_pinned_out"] = t
        # the same region from an unaligned origin that wraps both ways (funnel-shifted loads)
        t = timed(lambda: e.view_counts(37, 5, n // 64, n // 64, 64))
        t.update(origin=[37, 5], read_gbs_median=round(packed / t["median_ms"] / 1e6, 1),
                 read_gbs_best=round(packed / t["min_ms"] / 1e6, 1))
        res["whole_unaligned"] = t
        w1 = e.view_counts(12345, 4321, 1024, 1024, 1)
        assert np.array_equal(w1 * 255, e.store_rect(12345, 4321, 1024, 1024))
        t = timed(lambda: e.view_counts(12345, 4321, 1024, 1024, 1))
        t.update(board=n, scale=1, pixels=[1024, 1024], origin=[12345, 4321])
        res["window"] = t

    m = a.route_size
    with golhip.Engine(m, m, k=16) as e:
        e.init_random(3)
        via_store = block_sum(e.store(), 16)
        via_view = e.view_counts(0, 0, m // 16, m // 16, 16)
        assert np.array_equal(via_store, via_view), "the two routes disagree"
        store_t, sum_t, view_t = [], [], []
        for i in range(3 + 5):  # alternating, 3 warm rounds
            t0 = time.perf_counter()
            b = e.store()
            t1 = time.perf_counter()
            block_sum(b, 16)
            t2 = time.perf_counter()
            for _ in range(4):
                t3 = time.perf_counter()
                e.view_counts(0, 0, m // 16, m // 16, 16)
                if i >= 3:
                    view_t.append(time.perf_counter() - t3)
            if i >= 3:
                store_t.append(t1 - t0)
                sum_t.append(t2 - t1)
        ms = lambda ts: {"calls": len(ts), "median_ms": round(statistics.median(ts) * 1e3, 3),  # noqa: E731
                         "min_ms": round(min(ts) * 1e3, 3)}
        res["route"] = {"board": m, "scale": 16, "store_bytes": m * m, "store": ms(store_t),
                        "numpy_block_sum": ms(sum_t), "view_counts": ms(view_t),
                        "store_plus_sum_over_view": round((statistics.median(store_t) + statistics.median(sum_t))
                                                          / statistics.median(view_t), 1)}
    line = json.dumps(res)
    print(line)
    if a.out:
        a.out.parent.mkdir(parents=True, exist_ok=True)
        a.out.write_text(line + "\n")


if __name__ == "__main__":
    main()
