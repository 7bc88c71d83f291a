"""The scenarios of the receive-timeout tests, shared by the CPU file (tests/test_receive_timeout_model.py: the model
against the reference specs' known answers) and the GPU file (tests/test_gpu_receive_timeout.py: the engine against
the known answers and the model)."""
from __future__ import annotations

import json
import pathlib

import numpy as np

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.engine import NO_SENDER

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "receive_timeout_kats.json").read_text())
TAGS = KATS["tags"]
SCENARIOS = {s["name"]: s for s in KATS["scenarios"]}
KAT_NAMES = tuple(SCENARIOS)
KAT_T = (1, 5)
N_KAT, ACTOR, HOST = 80, 37, 80   # (80 actors in buckets of 32: a partial last bucket)
COUNT_KEYS = ("delivered", "dead_letters", "unhandled", "emitted", "staged", "supersteps", "in_flight")
RT_KEYS = ("fired", "discarded", "set", "pending")
TIMER_KEYS = ("s", "tt", "id")        # slot 0: the typed spec's scheduleOnce; 1, 2: the Timers spec's two periodic timers
TRANSPARENT = ("TransparentTick", "Identify")
B = typed.Behaviors


def payload(msg: str) -> int:
    """'Name' or 'Name:arg' -> the u32 payload"""
    name, _, arg = msg.partition(":")
    return (TAGS[name] << 24) | int(arg or 0)


def mtype(name: str) -> typed.MessageType:
    return typed.MessageType(name, TAGS[name])


def target_behavior(variant: str, delay: int) -> typed.Behavior:
    """The actors of ReceiveTimeoutSpec and ActorContextSpec as one behaviour.  ReceiveTimeout echoes GotTimeout to
    the monitor (the host id HOST) and is counted (state word 0); TransparentTick is counted (word 1); what else the
    two handlers do is the scenario's `variant`:
      plain          nothing more
      off            ReceiveTimeout also turns the timeout off                              (Spec :96-117)
      self_tt        ReceiveTimeout sends the actor a TransparentTick instead of the echo   (:154-170)
      tt_sets        TransparentTick sets the timeout to `delay`                            (:196-210)
      tt_cancels     TransparentTick turns it off                                           (:212-228, :230-247)
      tt_sets_twice  TransparentTick sets 2 x delay, counts, sets delay                      (:249-278)
    SetTimeout(d) sets the timeout and echoes TimeoutSet, Ping echoes Pong, Schedule starts a single timer of 10
    ticks whose message echoes Scheduled (ActorContextSpec :565-610); Tick and Identify do nothing; Stop stops."""
    host = typed.actor_ref(HOST)
    st = typed.State("timeouts", "tts")
    timeout = mtype("Timeout")
    ctx = typed.context

    def build(timers):
        for k in TIMER_KEYS:
            timers.cancel(k)  # (the keys, in slot order)
        on_timeout = {
            "off": lambda m, s: [s.timeouts.inc(), ctx.cancel_receive_timeout(), host.tell(mtype("GotTimeout")()), B.same],
            "self_tt": lambda m, s: [s.timeouts.inc(), typed.self_ref().tell(mtype("TransparentTick")()), B.same],
        }.get(variant, lambda m, s: [s.timeouts.inc(), host.tell(mtype("GotTimeout")()), B.same])
        on_tt = {
            "tt_sets": lambda m, s: [s.tts.inc(), ctx.set_receive_timeout(delay, timeout()), B.same],
            "tt_cancels": lambda m, s: [s.tts.inc(), ctx.cancel_receive_timeout(), B.same],
            "tt_sets_twice": lambda m, s: [ctx.set_receive_timeout(2 * delay, timeout()), s.tts.inc(),
                                           ctx.set_receive_timeout(delay, timeout()), B.same],
        }.get(variant, lambda m, s: [s.tts.inc(), B.same])
        return (typed.ReceiveBuilder.create(st)
                .on_message(timeout, on_timeout)
                .on_message(mtype("TransparentTick"), on_tt)
                .on_message(mtype("Tick"), lambda m, s: [B.same])
                .on_message(mtype("Identify"), lambda m, s: [B.same])
                .on_message(mtype("SetTimeout"), lambda m, s: [ctx.set_receive_timeout(m.arg, timeout()),
                                                               host.tell(mtype("TimeoutSet")()), B.same])
                .on_message(mtype("Ping"), lambda m, s: [host.tell(mtype("Pong")()), B.same])
                .on_message(mtype("Schedule"), lambda m, s: [timers.start_single_timer("s", mtype("Scheduled")(), 10), B.same])
                .on_message(mtype("Scheduled"), lambda m, s: [host.tell(mtype("Scheduled")()), B.same])
                .on_message(mtype("Stop"), lambda m, s: [B.stopped])
                .on_any_message(lambda m, s: [B.unhandled])
                .build("target_" + variant))
    return B.with_timers(build)


def target_workload(variants, delay: int, T: int, initial=(), timers=(), capacity: int = 0, ranges=None) -> wl.Workload:
    """N_KAT actors of target_behavior(variant, delay) -- `variants`: one name, or several with `ranges` = [(first,
    count, variant)]; `initial`: the setup block's (first, count, delay, message) sets; `timers`: (actor, slot,
    period, message) periodic starts."""
    names = [variants] if isinstance(variants, str) else list(variants)
    behs = {v: target_behavior(v, delay) for v in names}
    tb = typed.compile_behaviors(list(behs.values()), max_emit=1, transparent=[mtype(n) for n in TRANSPARENT])
    assert tb.uses_receive_timeout and tb.timer_keys == len(TIMER_KEYS)
    starts = [(a, 1, key, True, period, None, payload(msg)) for a, key, period, msg in timers]
    rt = {"transparent": tb.transparent_tags, "starts": [(f, c, d, payload(m)) for f, c, d, m in initial]}
    reg = [(f, c, tb.kind_of(behs[v]), None) for f, c, v in (ranges or [(0, N_KAT, names[0])])]
    return wl.Workload("receive_timeout_target", N_KAT, 2, 1, T, capacity, reg, behaviors=tb, outbound=(HOST, 1),
                       bucket_actors=32, timers={"n_keys": tb.timer_keys, "starts": starts, "receive_timeout": rt})


def become_workload(T: int, delay: int) -> wl.Workload:
    """two behaviours that become each other on Become; ReceiveTimeout echoes GotTimeout in the first, GotTimeoutB in
    the second; Stop stops.  The setup block sets the timeout of ACTOR: a become keeps it, a stop turns it off."""
    host = typed.actor_ref(HOST)
    st = typed.State("timeouts", "unused")
    first, second = typed.Behavior("first", st), typed.Behavior("second", st)
    for beh, got, nxt in ((first, "GotTimeout", second), (second, "GotTimeoutB", first)):
        (typed.ReceiveBuilder.create(st)
         .on_message(mtype("Timeout"), lambda m, s, got=got: [s.timeouts.inc(), host.tell(mtype(got)()), B.same])
         .on_message(mtype("Become"), lambda m, s, nxt=nxt: [nxt])
         .on_message(mtype("Stop"), lambda m, s: [B.stopped])
         .on_message(mtype("SetTimeout"), lambda m, s: [typed.context.set_receive_timeout(m.arg, mtype("Timeout")()), B.same])
         .on_any_message(lambda m, s: [B.unhandled])
         .build(into=beh))
    tb = typed.compile_behaviors([first], max_emit=1)
    assert tb.uses_receive_timeout and tb.timer_keys == 0   # (only a receive timeout: the engine still needs one key)
    return wl.Workload("receive_timeout_become", N_KAT, 2, 1, T, 0, [(0, N_KAT, tb.kind_of(first), None)], behaviors=tb,
                       outbound=(HOST, 1), bucket_actors=32,
                       timers={"n_keys": max(tb.timer_keys, 1),
                               "receive_timeout": {"transparent": (), "starts": [(ACTOR, 1, delay, payload("Timeout"))]}})


def kat_workload(name: str, T: int) -> wl.Workload:
    su = SCENARIOS[name]["setup"]
    return target_workload(su["variant"], su["delay"], T, initial=[(ACTOR, 1, su["delay"], "Timeout")] if su["initial"] else [],
                           timers=[(ACTOR, key, period, msg) for key, period, msg in su.get("timers", ())])


def counts(st) -> dict:
    return {k: (st[k] if isinstance(st, dict) else getattr(st, k)) for k in COUNT_KEYS}


def conserved(st: dict, timer_info: dict, rt_info: dict) -> bool:
    """staged + emitted + timer fired + receive-timeout fired = delivered + dead_letters + in_flight"""
    return st["staged"] + st["emitted"] + timer_info["fired"] + rt_info["fired"] == \
        st["delivered"] + st["dead_letters"] + st["in_flight"]


def run_kat(name: str, T: int, target) -> dict:
    """Run the scenario's script on `target` (an engine or the model, the workload applied): per step the echoes
    and the ticks, then the final counters, the two infos, the actor's timeout and its state words."""
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
        assert conserved(st, target.timer_info(), target.receive_timeout_info()), (name, T, st)
    info = target.receive_timeout_info()
    slot = target.read_receive_timeout(ACTOR, 1)
    words, alive = target.read_state()
    return dict(echo=echo, ticks=ticks, counts=st, info={k: info[k] for k in RT_KEYS}, timer_info=target.timer_info(),
                alive=int(alive[ACTOR] & 1), slot={k: int(slot[k][0]) for k in ("delay", "remaining", "payload")},
                words=[int(words[ACTOR, 0]), int(words[ACTOR, 1])])


def per_T(v, T: int):
    """a value of the JSON that differs by throughput is written {"1": .., "5": ..}"""
    return v[str(T)] if isinstance(v, dict) and set(v) == {"1", "5"} else v


def check_kat(name: str, T: int, got: dict) -> None:
    """`got` against the JSON."""
    sc = SCENARIOS[name]
    assert got["echo"] == [[payload(m) for m in e] for e in per_T(sc["echo"], T)], (got["echo"], sc["echo"])
    assert got["ticks"] == per_T(sc["ticks"], T), (got["ticks"], sc["ticks"])
    f = sc["final"]
    assert got["info"] == {k: per_T(f[k], T) for k in RT_KEYS}, got["info"]
    assert got["alive"] == f["alive"] and got["counts"]["dead_letters"] == per_T(f["dead_letters"], T), got
    assert got["counts"]["in_flight"] == 0
    assert {k: got["slot"][k] for k in f["slot"]} == {k: per_T(v, T) for k, v in f["slot"].items()}, got["slot"]
    assert got["words"] == per_T(f["words"], T), got["words"]
