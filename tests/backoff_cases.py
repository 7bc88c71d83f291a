"""The scenarios of the backoff tests, shared by the CPU files (tests/test_backoff_model.py: the model against the
reference spec's known answers) and the GPU files (tests/test_gpu_backoff.py: the engine against the known answers
and the model)."""
from __future__ import annotations

import json
import pathlib

import numpy as np

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.engine import NO_SENDER
from tests import supervision_cases as sc

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "backoff_kats.json").read_text())
TAGS = KATS["tags"]
SIGNALS = KATS["signals"]
CLASS_NAMES = tuple(KATS["classes"])
SCENARIOS = {s["name"]: s for s in KATS["scenarios"]}
KAT_NAMES = tuple(SCENARIOS)
KAT_T = (1, 3)
N_KAT, HOST, TARGET = 64, 64, 40
TICKER = (0, 1)   # the pair that keeps time flowing
COUNT_KEYS = sc.COUNT_KEYS
INFO_KEYS = sc.INFO_KEYS
BACKOFF_KEYS = ("backoffs", "resumed", "dropped", "limit_stops", "suspended")
B = typed.Behaviors
S = typed.SupervisorStrategy


def strategy(spec):
    """'resume' | 'stop' | 'restart' | [max_restarts, within] | {backoff: [min, max, q16], max_restarts, reset_after,
    stash} | a strategy"""
    if isinstance(spec, typed._Strategy):
        return spec
    if isinstance(spec, dict):
        mn, mx, q16 = spec["backoff"]
        return (S.restart_with_backoff(mn, mx, q16 / 65536.0).with_max_restarts(spec.get("max_restarts", -1))
                .with_reset_backoff_after(spec.get("reset_after", mn)).with_stash_capacity(spec.get("stash", -1)))
    return sc.strategy(spec)


def backoff(mn, mx, q16=0, max_restarts=-1, reset_after=None, stash=-1):
    return strategy(dict(backoff=[mn, mx, q16], max_restarts=max_restarts, reset_after=mn if reset_after is None else reset_after,
                         stash=stash))


def payload(msg: str) -> int:
    """'Name' or 'Name:arg' -> the u32 payload; the argument is a number, an exception class or a signal"""
    name, _, arg = msg.partition(":")
    a = CLASS_NAMES.index(arg) if arg in CLASS_NAMES else SIGNALS[arg] if arg in SIGNALS else int(arg or 0)
    return (TAGS[name] << 24) | a


def _is(t):
    return lambda m: m.tag == TAGS[t]


def target_behavior(sup, excs) -> typed.Behavior:
    """SupervisionSpec's targetBehavior (:56-86) as tests/supervision_cases has it, plus the ticker's Tick(k): k > 0
    answers the sender Tick(k - 1)."""
    host = typed.actor_ref(HOST)
    st = typed.State("n", "unused")
    rb = typed.ReceiveBuilder.create(st)
    rb.on_any_message(lambda m, s: [host.tell(m.arg, tag=TAGS["Pong"]), B.same], test=_is("Ping"))
    rb.on_any_message(lambda m, s: [s.n.inc(), B.same], test=_is("IncrementState"))
    rb.on_any_message(lambda m, s: [host.tell(s.n, tag=TAGS["State"]), B.same], test=_is("GetState"))
    rb.on_any_message(lambda m, s: [m.sender.tell(m.arg - 1, tag=TAGS["Tick"]), B.same], test=_is("Tick"),
                      when=lambda m, s: m.arg > 0)
    rb.on_any_message(lambda m, s: [B.same], test=_is("Tick"))
    for i, name in enumerate(CLASS_NAMES):
        rb.on_any_message(lambda m, s, e=excs[name]: [B.throw(e)], test=_is("Throw"), when=lambda m, s, i=i: m.arg == i)
    rb.on_any_message(lambda m, s: [B.unhandled])
    for sig, code in ((typed.PreRestart, SIGNALS["PreRestart"]), (typed.PostStop, SIGNALS["PostStop"])):
        rb.on_signal(sig, lambda g, s, code=code: [host.tell(code, tag=TAGS["ReceivedSignal"]), B.same])
    b = rb.build("target")
    for cls, spec in sup:
        b = B.supervise(b, reset={st.n: 0}).on_failure(strategy(spec), exc=excs[cls])
    return b


def workload_of(tb, name, n, T, kind, capacity=0, init=None, bucket_actors=32) -> wl.Workload:
    return wl.Workload(name, n, 2, 1, T, capacity, [(0, n, kind, init)], behaviors=tb, outbound=(n, 1),
                       bucket_actors=bucket_actors, supervision={"rows": tb.supervisors, "backoff": tb.backoff})


def kat_workload(name: str, T: int) -> wl.Workload:
    excs = sc.exception_types(KATS["classes"])
    b = target_behavior(SCENARIOS[name]["supervise"], excs)
    tb = typed.compile_behaviors([b], max_emit=1)
    return workload_of(tb, "backoff_kat", N_KAT, T, tb.kind_of(b))


def tick(target, ticks: int, pair=TICKER) -> None:
    """start the ticker pair: mail for exactly `ticks` supersteps"""
    target.tell(np.asarray([pair[0]], np.uint32), np.asarray([(TAGS["Tick"] << 24) | (ticks - 1)], np.uint32),
                np.asarray([pair[1]], np.uint32))


def counts(st) -> dict:
    return sc.counts(st)


def run_kat(name: str, T: int, target) -> dict:
    """Run the scenario's script on `target` (an engine or the model, the workload applied): per step the echoes,
    then the final counters and flags."""
    s = SCENARIOS[name]
    echo, st = [], None
    for step in s["script"]:
        p = np.asarray([payload(m) for m in step["tell"]], np.uint32)
        if p.size:
            target.tell(np.full(p.size, TARGET, np.uint32), p, np.full(p.size, NO_SENDER, np.uint32))
        tick(target, step["ticks"])
        st = counts(target.run(step["ticks"]))
        d, sd, p = target.take_outbound()
        assert (d == HOST).all() and (sd == TARGET).all()
        echo.append([int(x) for x in p])
    st = counts(target.run())  # (what is held is in flight: to quiescence)
    d, sd, p = target.take_outbound()
    assert p.size == 0
    info, bo = target.supervision_info(), target.backoff_info()
    _, alive = target.read_state()
    return dict(echo=echo, counts=st, info={k: info[k] for k in INFO_KEYS}, backoff={k: bo[k] for k in BACKOFF_KEYS},
                ticks=info["ticks"], alive=int(alive[TARGET] & 1),
                count=target.read_supervision(TARGET)["count"].tolist(), until=target.read_backoff(TARGET)["until"])


def check_kat(name: str, T: int, got: dict) -> None:
    """`got` against the JSON."""
    s = SCENARIOS[name]
    assert got["echo"] == [[payload(m) for m in e] for e in s["echo"]], (got["echo"], s["echo"])
    f = s["final"]
    assert got["info"] == {k: f[k] for k in INFO_KEYS}, got["info"]
    assert got["backoff"] == {k: f[k] for k in BACKOFF_KEYS}, got["backoff"]
    assert got["alive"] == f["alive"]
    assert got["count"][:len(f["count"])] == f["count"], got["count"]
    c = got["counts"]
    assert got["ticks"] == c["supersteps"] and c["in_flight"] == 0
    assert c["dead_letters"] >= f["dropped"]
    assert c["staged"] + c["emitted"] == c["delivered"] + c["dead_letters"] + c["in_flight"]


# ------------------------------------------------------------------ the shared workloads of the model and GPU tests
MIX_THROW, MIX_STOP, MIX_INC, MIX_ECHO, MIX_PRE, MIX_POST, MIX_TICK, MIX_TO = 1, 2, 4, 5, 6, 7, 9, 10
MIX_CLASSES = {"E1": None, "E2": "E1", "E3": None}
E1, E2, E3 = 0, 1, 2


def mix_behavior(host_id: int, sup, excs) -> typed.Behavior:
    """Throw(class) / Stop / Inc / Echo / Tick(k) / To(arg) by message.  Inc counts (word 0, which a restart resets) and
    keeps the payload (word 1); Echo tells the host the count; Tick(k > 0) answers the sender Tick(k - 1); To(arg)
    passes Inc(arg) to the actor named in word 1 (a sender whose messages race a bound: word 1 is then a constructor
    argument nobody overwrites, the actor gets no Inc).  Signals are echoed with the count of that moment."""
    host = typed.actor_ref(host_id)
    st = typed.State("n", "last")
    is_ = lambda t: (lambda m: m.tag == t)
    rb = typed.ReceiveBuilder.create(st)
    for i, name in enumerate(MIX_CLASSES):
        rb.on_any_message(lambda m, s, e=excs[name]: [B.throw(e)], test=is_(MIX_THROW), when=lambda m, s, i=i: m.arg == i)
    rb.on_any_message(lambda m, s: [B.stopped], test=is_(MIX_STOP))
    rb.on_any_message(lambda m, s: [s.n.inc(), s.last.set(m.payload), B.same], test=is_(MIX_INC))
    rb.on_any_message(lambda m, s: [host.tell(s.n, tag=MIX_ECHO), B.same], test=is_(MIX_ECHO))
    rb.on_any_message(lambda m, s: [m.sender.tell(m.arg - 1, tag=MIX_TICK), B.same], test=is_(MIX_TICK),
                      when=lambda m, s: m.arg > 0)
    rb.on_any_message(lambda m, s: [B.same], test=is_(MIX_TICK))
    rb.on_any_message(lambda m, s: [s.last.ref.tell(m.arg, tag=MIX_INC), B.same], test=is_(MIX_TO))
    rb.on_any_message(lambda m, s: [B.unhandled])
    rb.on_signal(typed.PreRestart, lambda g, s: [host.tell(s.n, tag=MIX_PRE), B.same])
    rb.on_signal(typed.PostStop, lambda g, s: [host.tell(s.n, tag=MIX_POST), B.same])
    b = rb.build("mix")
    for cls, spec in sup:
        b = B.supervise(b, reset={st.n: 0}).on_failure(strategy(spec), exc=excs[cls])
    return b


def mix_workload(n: int, T: int, sup, capacity: int = 0, init=None, bucket_actors: int = 32) -> wl.Workload:
    b = mix_behavior(n, sup, sc.exception_types(MIX_CLASSES))
    tb = typed.compile_behaviors([b], max_emit=1)
    init = np.zeros((n, 2), np.uint64) if init is None else init
    return workload_of(tb, "backoff_mix", n, T, tb.kind_of(b), capacity, init, bucket_actors)


def tells(target, *msgs, src=NO_SENDER):
    """(dst, tag, arg) ..., staged in this order"""
    d = np.asarray([m[0] for m in msgs], np.uint32)
    p = np.asarray([(m[1] << 24) | m[2] for m in msgs], np.uint32)
    target.tell(d, p, np.full(d.size, src, np.uint32))


def mix_tick(target, ticks: int, pair) -> None:
    target.tell(np.asarray([pair[0]], np.uint32), np.asarray([(MIX_TICK << 24) | (ticks - 1)], np.uint32),
                np.asarray([pair[1]], np.uint32))


def snapshot(target, actors) -> dict:
    """everything the GPU tests compare bit for bit"""
    s = sc.snapshot(target, actors)
    s["backoff"] = target.backoff_info()
    s["bo"] = [tuple(sorted(target.read_backoff(a).items())) for a in actors]
    return s
