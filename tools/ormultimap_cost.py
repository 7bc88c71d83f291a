#!/usr/bin/env python3
"""Device time per tick of ORMultiMap replicas in steady gossip, and of as many PNCounterMap
replicas beside it for scale, from agx_run_timed: a warm-up engine first, then on a fresh engine one settling window
and five measured windows of `--ticks` ticks each; the median window, the windows, messages per second and the
algorithmic bytes per tick, as JSON.

  python tools/ormultimap_cost.py ormultimap --n 262144 --msg-capacity 1048576     # workloads.crdt_ormultimap(n, fanout=2)
  python tools/ormultimap_cost.py pncountermap --n 262144 --msg-capacity 1048576   # workloads.crdt_pncountermap(n, fanout=2)

`--msg-capacity` is explicit: the row heap is 2 x (n rounded to buckets + msg_capacity) rows of 20608 B for
ORMultiMap replicas (54 GB at the sizes above; 10368 B and 27 GB for PNCounterMap), and the default capacity of
max(4n, 65536) is sized for small rows.

Algorithmic bytes per tick (ormultimap): every replica has work in every tick -- its state is read once and written
once (2576 u64), it writes one snapshot row and reads `fanout` rows, rows at their used length (32 + live key dots
rounded up to 4 + 72 per live key, u32), taken from the states at the end of the run; envelopes at 12 B in and out.
The same for pncountermap with 1296 u64 of state and 32 u32 per live key.  The state counted as written in full is an
upper bound: the kernels store key dots, values and version vector only where they changed.
"""
import argparse
import json
import pathlib
import statistics
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

HBM_PEAK = 8.0e12  # B/s (MI355X)
KEY_U32 = {"ormultimap": 72, "pncountermap": 32}


def workload(case: str, n: int, ticks: int, windows: int):
    from akka_amd import workloads as wl
    rounds = ticks * (windows + 1) + 64
    if case == "ormultimap":
        return wl.crdt_ormultimap(n, rounds=rounds, fanout=2)
    return wl.crdt_pncountermap(n, rounds=rounds, fanout=2)


def row_u32(case: str, words: np.ndarray) -> float:
    """Mean used length (u32) of a snapshot row of the replicas `words`."""
    dots = np.ascontiguousarray(words[:, :256]).view(np.uint32).reshape(len(words), 64, 8) != 0
    live = dots.sum(axis=(1, 2))
    keys = dots.any(axis=2).sum(axis=1)
    return float((32 + (live + 3) // 4 * 4 + KEY_U32[case] * keys).mean())


def run(case: str, n: int, cap: int, ticks: int, n_windows: int, measure_rows: bool):
    from akka_amd.engine import EngineConfig, GpuEngine
    w = workload(case, n, ticks, n_windows)
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), msg_capacity=cap)))
    w.apply_to(eng)
    ms, delivered = [], []
    last = 0
    for _ in range(n_windows):
        st, t = eng.run_timed(ticks)[:2]
        ms.append(t / ticks)
        delivered.append((st.delivered - last) / ticks)
        last = st.delivered
    rows = None
    if measure_rows:
        words, _ = eng.read_state()
        rows = row_u32(case, words[: 1 << 12])
    eng.close()
    return ms, delivered, rows, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["ormultimap", "pncountermap"])
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--msg-capacity", type=int, required=True)
    ap.add_argument("--ticks", type=int, default=32)
    ap.add_argument("--windows", type=int, default=5)
    a = ap.parse_args()
    run(a.case, a.n, a.msg_capacity, 4, 1, False)  # the warm-up engine
    ms, dl, rows, w = run(a.case, a.n, a.msg_capacity, a.ticks, a.windows + 1, True)
    meas, per_tick = ms[1:], dl[1:]  # (the first window settles: the writers' ops, the first rounds of gossip)
    med = statistics.median(meas)
    fanout = w.gossip[0]
    state_b = 8 * w.n_words
    alg = a.n * (2 * state_b + 4 * rows * (1 + fanout)) + 12 * 2 * statistics.median(per_tick)
    print(json.dumps(dict(case=a.case, n=a.n, msg_capacity=a.msg_capacity, ticks=a.ticks, ms_per_tick_median=med, windows=meas,
                          settling=ms[0], delivered_per_tick=statistics.median(per_tick),
                          msg_per_s=statistics.median(per_tick) / (med * 1e-3), row_u32_mean=rows, state_bytes=state_b,
                          alg_bytes_per_tick=alg, alg_bytes_per_s=alg / (med * 1e-3),
                          fraction_of_hbm_peak=alg / (med * 1e-3) / HBM_PEAK, state_total_bytes=a.n * state_b)))


if __name__ == "__main__":
    main()
