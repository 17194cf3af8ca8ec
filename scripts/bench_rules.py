#!/usr/bin/env python3
"""Rates of the life-like rule kernel (gol_rule) against the production B3/S23 path, one session, one
pre-heated chip: per board size one engine per leg on the same seeded board (seed 3), every launch
exactly 8 generations deep (set_k(8) + set_fixed_k), rounds alternating the leg order; the time is
the HIP-event span of golhip_timing / golhip_kernel_time.  Legs:
  life   B3/S23 on the production path (the yardstick)
  const  HighLife B36/S23, the constant-folded kernel (launch kind 5, param 1)
  table  B38/S0236, the table form (launch kind 5, param 0)
Prints one JSON line (median GCUPS per leg and size, every round, the ratios to `life`) and writes
it to --out.  The measurement runs in a child process under `timeout`.
--life-only runs the `life` leg alone and uses nothing of the rule interface, so the same file also
measures the yardstick on a checkout that predates it (--pkg DIR: that checkout's
distributed-gol_amd).
Usage: bench_rules.py [--sizes 16384,65536] [--rounds 7] [--gens 192] [--out FILE] [--life-only]
                      [--pkg DIR] [--timeout SECONDS]"""
import argparse
import json
import statistics
import subprocess
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parents[1]
K = 8
LEGS = {"life": "B3/S23", "const": "B36/S23", "table": "B38/S0236"}


def measure(args):
    sys.path.insert(0, args.pkg or str(ROOT / "distributed-gol_amd"))
    import golhip

    result = {"k": K, "seed": 3, "gens_per_sample": args.gens, "sizes": {}}
    for size in args.sizes:
        engines = {}
        for leg, rule in LEGS.items():
            if leg == "life":
                engines[leg] = golhip.Engine(size, size, k=K)
            elif not args.life_only:
                engines[leg] = golhip.Engine(size, size, k=K, rule=rule)
                want = ("rule", 1 if leg == "const" else 0)
                assert engines[leg].launch_kind(K) == want, (leg, engines[leg].launch_kind(K))
        for e in engines.values():
            e.set_fixed_k(True)
            e.init_random(3)
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 1.0:  # pre-heat the chip on every engine's kernels
            for e in engines.values():
                e.step(args.gens)  # the timed call itself: its graphs are captured here, not in a round
                e.sync()
        rounds = {leg: [] for leg in engines}
        for rnd in range(args.rounds):
            order = list(engines.items()) if rnd % 2 == 0 else list(reversed(engines.items()))
            for leg, e in order:
                e.timing(True)
                e.step(args.gens)
                e.sync()
                ms, launches, gens = e.kernel_time()
                e.timing(False)
                assert gens == args.gens and launches == args.gens // K, (leg, launches, gens)
                rounds[leg].append(size * size * gens / (ms * 1e-3) / 1e9)
        med = {leg: statistics.median(v) for leg, v in rounds.items()}
        result["sizes"][str(size)] = {
            "gcups": {leg: round(v, 1) for leg, v in med.items()},
            "ratio_to_life": {leg: round(med[leg] / med["life"], 4) for leg in med if leg != "life"},
            "life_spread": round((max(rounds["life"]) - min(rounds["life"])) / med["life"], 4),
            "rounds": {leg: [round(x, 1) for x in v] for leg, v in rounds.items()},
            "alive": {leg: e.alive_count() for leg, e in engines.items()},
        }
        for e in engines.values():
            e.close()
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", type=lambda s: [int(x) for x in s.split(",")], default=[16384, 65536])
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--gens", type=int, default=192)
    ap.add_argument("--out", default="")
    ap.add_argument("--life-only", action="store_true")
    ap.add_argument("--pkg", default="")
    ap.add_argument("--timeout", type=int, default=240)
    ap.add_argument("--child", action="store_true")
    args = ap.parse_args()
    if args.gens % K:
        ap.error(f"--gens must be a multiple of {K}")
    if args.child:
        return measure(args)
    # the measurement in a fresh child under a time limit (this process never opens the GPU)
    cmd = ["timeout", "-k", "10", str(args.timeout), sys.executable, __file__, "--child"] + sys.argv[1:]
    sys.exit(subprocess.run(cmd).returncode)


if __name__ == "__main__":
    main()
