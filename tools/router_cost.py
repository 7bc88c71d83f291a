#!/usr/bin/env python3
"""Device time per tick of the router logics at 2^20 actors, from agx_run_timed: a warm-up engine
first, then on a fresh engine one settling window and five measured windows of `--ticks` ticks each, the tick's host
tells staged before its run(1); the median window and the windows' range, as JSON.

  python tools/router_cost.py service_pool            # the receptionist engine (any library: AKKA_AMD_LIB)
  python tools/router_cost.py service_pool_random     # ... with agx_set_router_logics(0) made and unused
  python tools/router_cost.py service_pool_hashed     # ... with one hashed key of factor 10, made and unused
  python tools/router_cost.py sticky_static           # sticky_sessions, factor 10, a static pool
  python tools/router_cost.py sticky_one_stop         # ... one worker of the hashed key stops per tick
  python tools/router_cost.py ring_build              # host wall time of agx_set_router_logics, 2^20 x 10 points
"""
import argparse
import json
import pathlib
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parents[1]))

N = 1 << 20


def workload(case: str, ticks: int):
    from akka_amd import workloads as wl
    total = ticks * 7 + 8
    if case.startswith("service_pool"):
        w = wl.service_pool(1024, N - 1024, ticks=total)
        if case == "service_pool_random":
            w.router_logics = {"hashed_keys_mask": 0, "seed": 1}
        if case == "service_pool_hashed":
            w.router_logics = {"hashed_keys_mask": 1, "virtual_nodes_factor": 10, "seed": 1}
        return w
    nc = nr = 1 << 17
    nw = N - nc - nr
    w = wl.sticky_sessions(n_clients=nc, n_routers=nr, n_workers=nw, virtual_nodes_factor=10, ticks=total, throughput=8)
    if case == "sticky_one_stop":  # worker t (left = 1) gets a Request from the host in tick t and stops
        w0 = nc + nr
        w.ranges[2][3][:total, 0] = 1
        req = (wl.SS_REQUEST << 24) | 1
        w.schedule = [(np.concatenate([d, np.asarray([w0 + t], np.uint32)]), np.concatenate([s, np.asarray([wl.NO_SENDER], np.uint32)]),
                       np.concatenate([p, np.asarray([req], np.uint32)])) for t, (d, s, p) in enumerate(w.schedule)]
    return w


def windows(w, ticks: int, n_windows: int):
    from akka_amd.engine import EngineConfig, GpuEngine
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    w.apply_to(eng)
    out, t = [], 0
    for _ in range(n_windows):
        ms = 0.0
        for _ in range(ticks):
            dst, src, pay = w.schedule[t]
            eng.tell(dst, pay, src)
            ms += eng.run_timed(1)[1]
            t += 1
        out.append(ms / ticks)
    info = dict(receptionist=eng.receptionist_info(), router=eng.router_info() if w.router_logics else None)
    eng.close()
    return out, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case")
    ap.add_argument("--ticks", type=int, default=64)
    a = ap.parse_args()
    import __graft_entry__ as g
    g.build_native()
    if a.case == "ring_build":
        from akka_amd import workloads as wl
        from akka_amd.engine import EngineConfig, GpuEngine
        w = wl.sticky_sessions(n_clients=1 << 17, n_routers=1 << 17, n_workers=N - (1 << 18), virtual_nodes_factor=10, ticks=1)
        rl, w.router_logics = w.router_logics, {}
        walls = []
        for _ in range(3):
            eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
            w.apply_to(eng)
            eng.read_listing(0)  # (the setup block's registrations are on the device)
            t0 = time.perf_counter()
            eng.set_router_logics(rl["hashed_keys_mask"], rl["virtual_nodes_factor"], rl["seed"])
            walls.append(time.perf_counter() - t0)
            size = eng.router_info()["ring_size"][0]
            eng.close()
        print(json.dumps(dict(case=a.case, wall_s=walls, ring_points=size)))
        return
    w = workload(a.case, a.ticks)
    windows(w, 4, 1)  # the warm-up engine
    ms, info = windows(w, a.ticks, 6)
    meas = ms[1:]  # (the first window settles)
    print(json.dumps(dict(case=a.case, ticks=a.ticks, ms_per_tick_median=statistics.median(meas), windows=meas, settling=ms[0],
                          info=info)))


if __name__ == "__main__":
    main()
