"""The scenarios of the timer tests, shared by the CPU file (tests/test_timer_model.py: the model against the
frozen oracle and the reference spec's known answers) and the GPU file (tests/test_gpu_timers.py: the engine
against the known answers and the model)."""
from __future__ import annotations

import json
import pathlib

import numpy as np

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.engine import NO_SENDER

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "timer_kats.json").read_text())
TAGS = KATS["tags"]
SCENARIOS = {s["name"]: s for s in KATS["scenarios"]}
KAT_NAMES = tuple(SCENARIOS)
KAT_T = (1, 5)
N_KAT, ACTOR, HOST = 64, 37, 64
COUNT_KEYS = ("delivered", "dead_letters", "unhandled", "emitted", "staged", "supersteps", "in_flight")
INFO_KEYS = ("fired", "discarded", "active", "pending")


def payload(msg: str) -> int:
    """'Name' or 'Name:arg' -> the u32 payload"""
    name, _, arg = msg.partition(":")
    return (TAGS[name] << 24) | int(arg or 0)


def target_behavior(interval: int) -> typed.Behavior:
    """TimerSpec's `target` (:45-84): Tick(n) echoes Tock(n) to the monitor (the host id HOST), Bump restarts the
    periodic timer "T" with Tick(n + 1), Cancel cancels it and echoes Cancelled, End stops the actor; Become
    switches to a behaviour that answers TockB (the timers survive it)."""
    host = typed.actor_ref(HOST)
    st = typed.State("n", "unused")
    B = typed.Behaviors
    tick = typed.MessageType("Tick", TAGS["Tick"])
    is_ = lambda t: (lambda m: m.tag == TAGS[t])

    def build(timers):
        first, second = typed.Behavior("target", st), typed.Behavior("target_b", st)
        for beh, tock, nxt in ((first, "Tock", second), (second, "TockB", first)):
            (typed.ReceiveBuilder.create(st)
             .on_any_message(lambda m, s, tock=tock: [host.tell(m.arg, tag=TAGS[tock]), B.same], test=is_("Tick"))
             .on_any_message(lambda m, s: [s.n.inc(), timers.start_timer_with_fixed_delay("T", tick(s.n), interval), B.same],
                             test=is_("Bump"))
             .on_any_message(lambda m, s: [timers.cancel("T"), host.tell(0, tag=TAGS["Cancelled"]), B.same],
                             test=is_("Cancel"))
             .on_any_message(lambda m, s: [B.stopped], test=is_("End"))
             .on_any_message(lambda m, s, nxt=nxt: [nxt], test=is_("Become"))
             .on_any_message(lambda m, s: [B.unhandled])
             .build(into=beh))
        return first
    return B.with_timers(build)


def kat_workload(name: str, T: int) -> wl.Workload:
    su = SCENARIOS[name]["setup"]
    b = target_behavior(su["delay"])
    tb = typed.compile_behaviors([b], max_emit=1)
    init = np.tile(np.asarray([1, 0], np.uint64), (N_KAT, 1))
    return wl.Workload("timer_kat", N_KAT, 2, 1, T, 0, [(0, N_KAT, tb.kind_of(b), init)], behaviors=tb,
                       outbound=(HOST, 1), bucket_actors=32,
                       timers={"n_keys": tb.timer_keys,
                               "starts": [(ACTOR, 1, 0, su["periodic"], su["delay"], None, payload("Tick:1"))]})


def counts(st) -> dict:
    return {k: (st[k] if isinstance(st, dict) else getattr(st, k)) for k in COUNT_KEYS}


def run_kat(name: str, T: int, target) -> dict:
    """Run the scenario's script on `target` (an engine or the model, the workload applied): per step the
    echoes and the ticks, then the final counters and slot."""
    sc = SCENARIOS[name]
    echo, ticks, st = [], [], None
    for step in sc["script"]:
        if step["tell"]:
            p = np.asarray([payload(m) for m in step["tell"]], np.uint32)
            target.tell(np.full(p.size, ACTOR, np.uint32), p, np.full(p.size, NO_SENDER, np.uint32))
        st = counts(target.run() if step["run"] is None else target.run(step["run"]))
        d, s, p = target.take_outbound()
        assert (d == HOST).all() and (s == ACTOR).all()
        echo.append([int(x) for x in p])
        ticks.append(target.timer_info()["ticks"])
    info = target.timer_info()
    slot = target.read_timers(ACTOR)
    _, alive = target.read_state()
    return dict(echo=echo, ticks=ticks, counts=st, info={k: info[k] for k in INFO_KEYS}, alive=int(alive[ACTOR] & 1),
                slot={k: int(slot[k][0]) for k in ("active", "remaining", "period", "payload", "generation")})


def check_kat(name: str, T: int, got: dict) -> None:
    """`got` against the JSON."""
    sc = SCENARIOS[name]
    assert got["echo"] == [[payload(m) for m in e] for e in sc["echo"]], (got["echo"], sc["echo"])
    assert got["ticks"] == sc["ticks"][str(T)], (got["ticks"], sc["ticks"])
    f = sc["final"]
    assert got["info"] == {k: f[k] for k in INFO_KEYS}, got["info"]
    assert got["alive"] == f["alive"] and got["counts"]["dead_letters"] == f["dead_letters"]
    assert {k: got["slot"][k] for k in f["slot"]} == f["slot"], got["slot"]
    c = got["counts"]  # conservation with `fired`
    assert c["staged"] + c["emitted"] + got["info"]["fired"] == c["delivered"] + c["dead_letters"] + c["in_flight"]
