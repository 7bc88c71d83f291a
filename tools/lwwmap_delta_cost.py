#!/usr/bin/env python3
"""Device time per tick and row bytes per tick of LWWMap replicas under delta replication, beside
full-state gossip of as many LWWMap replicas, from agx_run_timed: a warm-up engine first, then on a fresh engine one
settling window and five measured windows of `--ticks` ticks each; the median window, the windows, messages per second
and the row bytes written per tick, as JSON.

  python tools/lwwmap_delta_cost.py delta --n 262144       # workloads.crdt_lwwmap_delta(n, write=True): every tick one
                                                           # seeded update per replica and up to 2 DeltaPropagations
  python tools/lwwmap_delta_cost.py delta_gossip --n 262144  # the same with a full-state GossipTick (fanout 2) beside every tick
  python tools/lwwmap_delta_cost.py full --n 262144        # workloads.crdt_lwwmap(n, fanout=2): every tick one snapshot row
                                                           # per replica, told to 2 peers

Recorded runs: profiles/r30/ (README.md there names each command line and its output file).

Row bytes written per tick.  full: one snapshot row per replica at its used length (32 + live dots + 3 per live key,
u32), from the states at the end of the run.  delta: the DeltaPropagation rows of the model's run of the same workload
over `--model-n` replicas (keys of 8 replicas are independent of each other, so the mean per replica and tick does not
depend on n): told rows at their used length, 12 + 5 per put + 9 per remove u32; placeholder groups write 12 u32.
"""
import argparse
import json
import pathlib
import statistics
import sys

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))


def workload(case: str, n: int, rounds: int):
    from akka_amd import workloads as wl
    if case == "full":
        return wl.crdt_lwwmap(n, rounds=rounds, fanout=2)
    return wl.crdt_lwwmap_delta(n, rounds=rounds, write=True, gossip_rounds=rounds if case == "delta_gossip" else 0, fanout=2)


def full_row_u32(words: np.ndarray) -> float:
    dots = np.ascontiguousarray(words[:, :256]).view(np.uint32).reshape(len(words), 64, 8) != 0
    return float((32 + dots.sum(axis=(1, 2)) + 3 * dots.any(axis=2).sum(axis=1)).mean())


def delta_row_bytes(case: str, n: int, ticks: int) -> dict:
    """Per replica and tick, on the model: DeltaPropagation rows told and their mean used length."""
    from tests import lwwmap_delta_model as D
    w = workload(case, n, ticks)
    m = D.LwwDeltaModel(**w.engine_kwargs())
    told = []
    tick = m._tick

    def spy(a, arg, out):
        k = len(out)
        tick(a, arg, out)
        for dst, src, pay in out[k:]:
            if src == D.WIDE and pay[0] == "delta":
                told.append(12 + sum(5 if isinstance(o, D.PutDeltaOp) else 9 for o in D.delta_ops(pay[4])))

    m._tick = spy
    w.apply_to(m)
    m.run()
    rows = len(told) + m.census["placeholders"]
    u32 = sum(told) + 12 * m.census["placeholders"]
    return dict(model_n=n, model_ticks=ticks, rows_per_replica_tick=rows / (n * ticks), u32_per_row_mean=u32 / max(rows, 1),
                row_bytes_per_replica_tick=4 * u32 / (n * ticks), placeholders=m.census["placeholders"])


def run(case: str, n: int, cap: int, ticks: int, n_windows: int):
    from akka_amd.engine import EngineConfig, GpuEngine
    w = workload(case, n, ticks * n_windows + 64)
    eng = GpuEngine(EngineConfig(**dict(w.gpu_kwargs(), msg_capacity=cap)))
    w.apply_to(eng)
    ms, delivered, last = [], [], 0
    for _ in range(n_windows):
        st, t = eng.run_timed(ticks)[:2]
        ms.append(t / ticks)
        delivered.append((st.delivered - last) / ticks)
        last = st.delivered
    words, _ = eng.read_state()
    eng.close()
    return ms, delivered, words[: 1 << 12]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["delta", "delta_gossip", "full"])
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--msg-capacity", type=int, default=1 << 21)
    ap.add_argument("--ticks", type=int, default=32)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--model-n", type=int, default=256)
    a = ap.parse_args()
    run(a.case, a.n, a.msg_capacity, 4, 1)  # the warm-up engine
    ms, dl, words = run(a.case, a.n, a.msg_capacity, a.ticks, a.windows + 1)
    meas, per_tick = ms[1:], dl[1:]  # (the first window settles)
    med = statistics.median(meas)
    out = dict(case=a.case, n=a.n, msg_capacity=a.msg_capacity, ticks=a.ticks, ms_per_tick_median=med, windows=meas,
               settling=ms[0], delivered_per_tick=statistics.median(per_tick),
               msg_per_s=statistics.median(per_tick) / (med * 1e-3))
    full_row = 4 * full_row_u32(words)
    if a.case == "full":
        out.update(row_bytes_per_replica_tick=full_row, row_bytes_per_tick=a.n * full_row)
    else:
        d = delta_row_bytes("delta", a.model_n, 24)
        per = d["row_bytes_per_replica_tick"] + (full_row + 32 if a.case == "delta_gossip" else 0)
        out.update(delta_rows=d, full_state_row_bytes=full_row + 32, row_bytes_per_replica_tick=per, row_bytes_per_tick=a.n * per)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
