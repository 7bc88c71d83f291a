"""The scenarios of the supervision tests, shared by the CPU file (tests/test_supervision_model.py: the model
against the frozen oracle and the reference spec's known answers) and the GPU file (tests/test_gpu_supervision.py:
the engine against the known answers and the model)."""
from __future__ import annotations

import json
import pathlib

import numpy as np

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.engine import NO_SENDER

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "supervision_kats.json").read_text())
TAGS = KATS["tags"]
SIGNALS = KATS["signals"]
CLASS_NAMES = tuple(KATS["classes"])
SCENARIOS = {s["name"]: s for s in KATS["scenarios"]}
KAT_NAMES = tuple(SCENARIOS)
KAT_T = (1, 3)
N_KAT, HOST, TARGET = 64, 64, 40
COUNT_KEYS = ("delivered", "dead_letters", "unhandled", "emitted", "staged", "supersteps", "in_flight")
INFO_KEYS = ("failures", "resumes", "restarts", "stops")
B = typed.Behaviors
S = typed.SupervisorStrategy


def exception_types(classes: dict) -> dict:
    """{name: parent name or None} -> {name: ExceptionType}, 'Throwable' included"""
    out = {"Throwable": typed.Throwable}
    for name, parent in classes.items():
        out[name] = typed.ExceptionType(name, out[parent] if parent else None)
    return out


def strategy(spec):
    """'resume' | 'stop' | 'restart' | [max_restarts, within]"""
    if isinstance(spec, str):
        return getattr(S, spec)
    return S.restart.with_limit(int(spec[0]), int(spec[1]))


def payload(msg: str) -> int:
    """'Name' or 'Name:arg' -> the u32 payload; the argument is a number, an exception class or a signal"""
    name, _, arg = msg.partition(":")
    a = CLASS_NAMES.index(arg) if arg in CLASS_NAMES else SIGNALS[arg] if arg in SIGNALS else int(arg or 0)
    return (TAGS[name] << 24) | a


def _is(t):
    return lambda m: m.tag == TAGS[t]


def target_behavior(sup, excs) -> typed.Behavior:
    """SupervisionSpec's targetBehavior (:56-86), the monitor being the host id HOST; `sup`: the supervisors, inner
    first.  A restart re-creates State(0)."""
    host = typed.actor_ref(HOST)
    st = typed.State("n", "unused")
    rb = typed.ReceiveBuilder.create(st)
    rb.on_any_message(lambda m, s: [host.tell(m.arg, tag=TAGS["Pong"]), B.same], test=_is("Ping"))
    rb.on_any_message(lambda m, s: [s.n.inc(), B.same], test=_is("IncrementState"))
    rb.on_any_message(lambda m, s: [host.tell(s.n, tag=TAGS["State"]), B.same], test=_is("GetState"))
    for i, name in enumerate(CLASS_NAMES):
        rb.on_any_message(lambda m, s, e=excs[name]: [B.throw(e)], test=_is("Throw"), when=lambda m, s, i=i: m.arg == i)
    rb.on_any_message(lambda m, s: [B.unhandled])
    for sig, code in ((typed.PreRestart, SIGNALS["PreRestart"]), (typed.PostStop, SIGNALS["PostStop"])):
        rb.on_signal(sig, lambda g, s, code=code: [host.tell(code, tag=TAGS["ReceivedSignal"]), B.same])
    b = rb.build("target")
    for cls, spec in sup:
        b = B.supervise(b, reset={st.n: 0}).on_failure(strategy(spec), exc=excs[cls])
    return b


def kat_workload(name: str, T: int) -> wl.Workload:
    excs = exception_types(KATS["classes"])
    b = target_behavior(SCENARIOS[name]["supervise"], excs)
    tb = typed.compile_behaviors([b], max_emit=1)
    return wl.Workload("supervision_kat", N_KAT, 2, 1, T, 0, [(0, N_KAT, tb.kind_of(b), None)], behaviors=tb,
                       outbound=(HOST, 1), bucket_actors=32, supervision={"rows": tb.supervisors})


def counts(st) -> dict:
    return {k: (st[k] if isinstance(st, dict) else getattr(st, k)) for k in COUNT_KEYS}


def run_kat(name: str, T: int, target) -> dict:
    """Run the scenario's script on `target` (an engine or the model, the workload applied): per step the echoes,
    then the final counters and flags."""
    sc = SCENARIOS[name]
    echo, st = [], None
    for step in sc["script"]:
        p = np.asarray([payload(m) for m in step], np.uint32)
        target.tell(np.full(p.size, TARGET, np.uint32), p, np.full(p.size, NO_SENDER, np.uint32))
        st = counts(target.run())
        d, s, p = target.take_outbound()
        assert (d == HOST).all() and (s == TARGET).all()
        echo.append([int(x) for x in p])
    info = target.supervision_info()
    _, alive = target.read_state()
    return dict(echo=echo, counts=st, info={k: info[k] for k in INFO_KEYS}, ticks=info["ticks"],
                alive=int(alive[TARGET] & 1))


def check_kat(name: str, T: int, got: dict) -> None:
    """`got` against the JSON."""
    sc = SCENARIOS[name]
    assert got["echo"] == [[payload(m) for m in e] for e in sc["echo"]], (got["echo"], sc["echo"])
    f = sc["final"]
    assert got["info"] == {k: f[k] for k in INFO_KEYS}, got["info"]
    assert got["alive"] == f["alive"]
    c = got["counts"]
    assert got["ticks"] == c["supersteps"] and c["in_flight"] == 0
    assert c["staged"] + c["emitted"] == c["delivered"] + c["dead_letters"] + c["in_flight"]


# ------------------------------------------------------------------ the shared workloads of the model and GPU tests
MIX_THROW, MIX_STOP, MIX_BECOME, MIX_INC, MIX_ECHO, MIX_PRE, MIX_POST, MIX_PASS = 1, 2, 3, 4, 5, 6, 7, 8
MIX_CLASSES = {"E1": None, "E2": "E1", "E3": None}
MIX_SUP = (("E1", [2, 3]),)   # restart.with_limit(2, 3) for E1 and its child E2; E3 is not caught


def mix_behavior(host_id: int, sup, excs) -> typed.Behavior:
    """Throw(class) / Stop / Become / Inc / Echo / Pass(hops) by message.  `first` is the supervised initial
    behaviour, `second` the one it becomes: it counts in tens, so the state shows which behaviour ran.  Signals are
    echoed to the host with the count the behaviour has at that moment (the state a restart is about to reset)."""
    host = typed.actor_ref(host_id)
    st = typed.State("n", "last")
    is_ = lambda t: (lambda m: m.tag == t)
    names = list(MIX_CLASSES)
    second = typed.Behavior("second", st)

    def fill(rb, step, become, base):
        for i, name in enumerate(names):
            rb.on_any_message(lambda m, s, e=excs[name]: [s.last.set(m.payload), B.throw(e)], test=is_(MIX_THROW),
                              when=lambda m, s, i=i: m.arg == i)
        rb.on_any_message(lambda m, s: [B.stopped], test=is_(MIX_STOP))
        if become is not None:
            rb.on_any_message(lambda m, s: [s.n.inc(step), become], test=is_(MIX_BECOME))
        rb.on_any_message(lambda m, s: [s.n.inc(step), s.last.set(m.payload), B.same], test=is_(MIX_INC))
        rb.on_any_message(lambda m, s: [host.tell(s.n, tag=MIX_ECHO + base), B.same], test=is_(MIX_ECHO))
        rb.on_any_message(lambda m, s: [s.n.inc(step), typed.self_ref(1).tell(m.payload - 1), B.same], test=is_(MIX_PASS),
                          when=lambda m, s: m.arg > 0)
        rb.on_any_message(lambda m, s: [B.unhandled])
        rb.on_signal(typed.PreRestart, lambda g, s: [host.tell(s.n, tag=MIX_PRE + base), B.same])
        rb.on_signal(typed.PostStop, lambda g, s: [host.tell(s.n, tag=MIX_POST + base), B.same])
        return rb

    fill(typed.ReceiveBuilder.create(st), 10, None, 16).build(into=second)
    first = fill(typed.ReceiveBuilder.create(st), 1, second, 0).build("first")
    for cls, spec in sup:
        first = B.supervise(first, reset={st.n: 0}).on_failure(strategy(spec), exc=excs[cls])
    return first


def mix_workload(n: int, T: int, sup=MIX_SUP, bucket_actors: int = 32, capacity: int = 0) -> wl.Workload:
    b = mix_behavior(n, sup, exception_types(MIX_CLASSES))
    tb = typed.compile_behaviors([b], max_emit=1)
    init = np.zeros((n, 2), np.uint64)
    return wl.Workload("supervision_mix", n, 2, 1, T, capacity, [(0, n, tb.kind_of(b), init)], behaviors=tb,
                       outbound=(n, 1), bucket_actors=bucket_actors, supervision={"rows": tb.supervisors})


def tells(target, *msgs):
    """(dst, tag, arg) ..., staged in this order"""
    d = np.asarray([m[0] for m in msgs], np.uint32)
    p = np.asarray([(m[1] << 24) | m[2] for m in msgs], np.uint32)
    target.tell(d, p, np.full(d.size, NO_SENDER, np.uint32))


def shapes_script(n: int):
    """failures in the first and the last actor of every bucket of 32 (the last one partial at 70), two failures of
    one actor inside one drain window (T = 3), a failure as the last message before a `stopped`, a restart after a
    become (the kind returns to the initial one), an uncaught class, and the limit of 2 within 3 ticks exceeded"""
    E1, E2, E3 = 0, 1, 2
    edge = sorted({0, 31, 32, 63, 64, n - 1})

    def script(t):
        tells(t, *[(a, MIX_INC, 7) for a in edge], *[(a, MIX_THROW, E1) for a in edge],
              (5, MIX_THROW, E1), (5, MIX_INC, 1), (5, MIX_THROW, E2),          # two failures in one window
              (6, MIX_INC, 1), (6, MIX_THROW, E1), (6, MIX_STOP, 0), (6, MIX_INC, 2),   # a failure, then stopped
              (7, MIX_BECOME, 0), (7, MIX_INC, 1), (7, MIX_THROW, E2),           # a restart after a become
              (8, MIX_INC, 3), (8, MIX_THROW, E3), (8, MIX_INC, 4),              # not caught: stops
              (9, MIX_PASS, 40), (n - 2, MIX_PASS, 5))                           # (mail that crosses the buckets)
        yield t.run(1)
        yield t.run(2)
        tells(t, (5, MIX_THROW, E1), *[(a, MIX_ECHO, 0) for a in (0, 5, 6, 7, 8, n - 1)], (7, MIX_INC, 1))
        yield t.run()
        tells(t, (7, MIX_BECOME, 0), (7, MIX_STOP, 0), (0, MIX_THROW, E1), (0, MIX_THROW, E1), (0, MIX_THROW, E1))
        yield t.run()
    return script


def snapshot(target, actors) -> dict:
    """everything the GPU tests compare bit for bit"""
    words, alive = target.read_state()
    info = target.supervision_info()
    d, s, p = target.take_outbound()
    o = np.argsort(s, kind="stable")
    sup = []
    for a in actors:
        r = target.read_supervision(a)
        sup.append((r["initial_kind"], r["count"].tolist(), r["remaining"].tolist()))
    return dict(words=words.tolist(), alive=(alive & 1).tolist(), info=info,
                outbox=np.stack([s[o], d[o], p[o]]).tolist(), sup=sup)
