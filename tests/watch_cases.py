"""The scenarios of the death watch tests, shared by the CPU file (tests/test_watch_model.py: the model against
the frozen oracle and the reference spec's known answers) and the GPU file (tests/test_gpu_watch.py: the engine
against the known answers and the model)."""
from __future__ import annotations

import json
import pathlib

import numpy as np

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.engine import NO_SENDER

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "watch_kats.json").read_text())
TAGS = KATS["tags"]
ACTORS = KATS["actors"]
SCENARIOS = {s["name"]: s for s in KATS["scenarios"]}
KAT_NAMES = tuple(SCENARIOS)
KAT_T = (1, 5)
N_KAT, HOST = 64, 64
COUNT_KEYS = ("delivered", "dead_letters", "unhandled", "emitted", "staged", "supersteps", "in_flight")
INFO_KEYS = ("watches", "terminated", "discarded", "death_pacts", "conflicts", "watching", "pending")
B = typed.Behaviors
ctx = typed.context


def payload(msg: str) -> int:
    """'Name' or 'Name:arg' -> the u32 payload"""
    name, _, arg = msg.partition(":")
    return (TAGS[name] << 24) | int(arg or 0)


def _is(t):
    return lambda m: m.tag == TAGS[t]


def terminator_behavior() -> typed.Behavior:
    """WatchSpec's terminatorBehavior (:30-32): Stop stops it."""
    return (typed.ReceiveBuilder.create(typed.State("n", "unused"))
            .on_any_message(lambda m, s: [B.stopped], test=_is("Stop"))
            .on_any_message(lambda m, s: [B.unhandled]).build("terminator"))


def watcher_behavior(kind: str) -> typed.Behavior:
    """The watchers of WatchSpec, echoing to the monitor (the host id HOST).  The watchee is the message's
    argument.  `signal` (WatchSetup, :54-74): StartWatching watches and answers Done, Terminated(ref) is echoed as
    Got(ref) and stops the watcher.  `with` (WatchWithSetup, :206-222): StartWatchingWith1/2 watchWith
    Custom1/2 and answer Done, any other message is echoed and stops the watcher.  `unwatch` (:242-299): as
    `with`, but the watchWith is preceded by an unwatch, and StartWatching watches.  `error` (ErrorTestSetup,
    :301-324): the three calls without an unwatch, anything else stops."""
    host = typed.actor_ref(HOST)
    st = typed.State("n", "unused")
    c1, c2 = typed.MessageType("Custom1", TAGS["Custom1"]), typed.MessageType("Custom2", TAGS["Custom2"])
    ref = lambda m: typed.Ref(m.arg)
    rb = typed.ReceiveBuilder.create(st)
    if kind == "signal":
        rb.on_any_message(lambda m, s: [ctx.watch(ref(m)), host.tell(0, tag=TAGS["Done"]), B.same], test=_is("StartWatching"))
        rb.on_any_message(lambda m, s: [B.unhandled])
        rb.on_signal(typed.Terminated, lambda sig, s: [host.tell(sig.ref.dst, tag=TAGS["Got"]), B.stopped])
    else:
        pre = (lambda m: [ctx.unwatch(ref(m))]) if kind == "unwatch" else (lambda m: [])
        done = [] if kind == "error" else [host.tell(0, tag=TAGS["Done"])]
        if kind != "with":
            rb.on_any_message(lambda m, s: [ctx.watch(ref(m)), B.same], test=_is("StartWatching"))
        for name, c in (("StartWatchingWith1", c1), ("StartWatchingWith2", c2)):
            rb.on_any_message(lambda m, s, c=c: pre(m) + [ctx.watch_with(ref(m), c(0))] + done + [B.same], test=_is(name))
        if kind == "error":
            rb.on_any_message(lambda m, s: [B.stopped])
        else:
            rb.on_any_message(lambda m, s: [host.tell(m.payload), B.stopped])
    return rb.build("watcher_" + kind)


def chain_behaviors():
    """The death pact's three actors (:155-194): the boss relays to middle management and handles Terminated
    (echoes Failed(ref), stops); middle management relays to Joe and handles nothing; Joe fails on any message."""
    host = typed.actor_ref(HOST)
    st = typed.State("next", "unused")
    boss = (typed.ReceiveBuilder.create(st)
            .on_any_message(lambda m, s: [s.next.ref.tell(m.payload), B.same])
            .on_signal(typed.Terminated, lambda sig, s: [host.tell(sig.ref.dst, tag=TAGS["Failed"]), B.stopped])
            .build("boss"))
    middle = (typed.ReceiveBuilder.create(st)
              .on_any_message(lambda m, s: [s.next.ref.tell(m.payload), B.same]).build("middle"))
    joe = typed.ReceiveBuilder.create(st).on_any_message(lambda m, s: [B.stopped]).build("joe")
    return boss, middle, joe


def kat_workload(name: str, T: int) -> wl.Workload:
    kind = SCENARIOS[name]["setup"]
    A = ACTORS
    term = terminator_behavior()
    if kind == "chain":
        boss, middle, joe = chain_behaviors()
        tb = typed.compile_behaviors([term, boss, middle, joe], max_emit=1)
        nxt = lambda x: np.asarray([[x, 0]], np.uint64)
        ranges = [(0, N_KAT, tb.kind_of(term), None), (A["boss"], 1, tb.kind_of(boss), nxt(A["middle"])),
                  (A["middle"], 1, tb.kind_of(middle), nxt(A["joe"])), (A["joe"], 1, tb.kind_of(joe), None)]
        starts = [(A["middle"], 1, [A["joe"]], 0, None), (A["boss"], 1, [A["middle"]], 0, None)]
    else:
        w = watcher_behavior(kind)
        tb = typed.compile_behaviors([term, w], max_emit=1)
        ranges = [(0, N_KAT, tb.kind_of(term), None), (A["watcher"], 1, tb.kind_of(w), None)]
        starts = []
    return wl.Workload("watch_kat", N_KAT, 2, 1, T, 0, ranges, behaviors=tb, outbound=(HOST, 1), bucket_actors=32,
                       watch={"n_slots": 2, "starts": starts})


def counts(st) -> dict:
    return {k: (st[k] if isinstance(st, dict) else getattr(st, k)) for k in COUNT_KEYS}


def run_kat(name: str, T: int, target) -> dict:
    """Run the scenario's script on `target` (an engine or the model, the workload applied): per step the
    echoes and the ticks, then the final counters, flags and slots."""
    sc = SCENARIOS[name]
    echo, ticks, st = [], [], None
    for step in sc["script"]:
        if step["tell"]:
            d = np.asarray([ACTORS[a] for a, _ in step["tell"]], np.uint32)
            p = np.asarray([payload(m) for _, m in step["tell"]], np.uint32)
            target.tell(d, p, np.full(p.size, NO_SENDER, np.uint32))
        st = counts(target.run() if step["run"] is None else target.run(step["run"]))
        d, s, p = target.take_outbound()
        assert (d == HOST).all()
        echo.append([[int(a), int(x)] for a, x in zip(s, p)])
        ticks.append(target.watch_info()["ticks"])
    info = target.watch_info()
    _, alive = target.read_state()
    slots = {a: {k: v.tolist() for k, v in target.read_watch(ACTORS[a]).items()} for a in sc["final"]["alive"]}
    return dict(echo=echo, ticks=ticks, counts=st, info={k: info[k] for k in INFO_KEYS},
                alive={a: int(alive[ACTORS[a]] & 1) for a in sc["final"]["alive"]}, slots=slots)


def check_kat(name: str, T: int, got: dict) -> None:
    """`got` against the JSON."""
    sc = SCENARIOS[name]
    assert got["echo"] == [[[ACTORS[a], payload(m)] for a, m in e] for e in sc["echo"]], (got["echo"], sc["echo"])
    assert got["ticks"] == sc["ticks"][str(T)], (got["ticks"], sc["ticks"])
    f = sc["final"]
    assert got["info"] == {k: f[k] for k in INFO_KEYS}, got["info"]
    assert got["alive"] == f["alive"], got["alive"]
    c = got["counts"]  # conservation with `terminated`
    assert c["in_flight"] == 0 and c["dead_letters"] == f["dead_letters"]
    assert c["staged"] + c["emitted"] + got["info"]["terminated"] == c["delivered"] + c["dead_letters"] + c["in_flight"]


# ------------------------------------------------------------------ the shared workloads of the model and GPU tests
MIX_WATCH, MIX_UNWATCH, MIX_STOP, MIX_WITH, MIX_DOWN, MIX_ECHO = 1, 2, 3, 4, 5, 6


def mix_behavior(host_id: int) -> typed.Behavior:
    """Watch(x) / WatchWith(x) / Unwatch(x) / Stop by message, x the argument; a Terminated or a Down is counted
    and echoed to the host with the terminated ref."""
    host = typed.actor_ref(host_id)
    st = typed.State("seen", "last")
    down = typed.MessageType("Down", MIX_DOWN)
    ref = lambda m: typed.Ref(m.arg)
    is_ = lambda t: (lambda m: m.tag == t)
    return (typed.ReceiveBuilder.create(st)
            .on_any_message(lambda m, s: [ctx.unwatch(ref(m)), ctx.watch(ref(m)), B.same], test=is_(MIX_WATCH))
            .on_any_message(lambda m, s: [ctx.unwatch(ref(m)), ctx.watch_with(ref(m), down(m.arg)), B.same], test=is_(MIX_WITH))
            .on_any_message(lambda m, s: [ctx.unwatch(ref(m)), B.same], test=is_(MIX_UNWATCH))
            .on_any_message(lambda m, s: [B.stopped], test=is_(MIX_STOP))
            .on_any_message(lambda m, s: [s.seen.inc(), s.last.set(m.sender.dst), host.tell(m.sender.dst, tag=MIX_DOWN), B.same],
                            test=is_(MIX_DOWN))
            .on_any_message(lambda m, s: [B.unhandled])
            .on_signal(typed.Terminated, lambda sig, s: [s.seen.inc(), s.last.set(sig.ref.dst),
                                                         host.tell(sig.ref.dst, tag=MIX_ECHO), B.same])
            .build("mix"))


def mix_workload(n: int, T: int, bucket_actors: int = 32, n_slots: int = 4, capacity: int = 0) -> wl.Workload:
    b = mix_behavior(n)
    tb = typed.compile_behaviors([b], max_emit=1)
    return wl.Workload("watch_mix", n, 2, 1, T, capacity, [(0, n, tb.kind_of(b), None)], behaviors=tb, outbound=(n, 1),
                       bucket_actors=bucket_actors, watch={"n_slots": n_slots})


def mix_rounds(n: int, seed: int, rounds: int = 6, per_round: int = 40):
    """(dst, payload) per round: a random mix of watch / watchWith / unwatch / stop messages over few watchees,
    so slots are reused, watchees are dead already, and unwatches race Terminated envelopes"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(rounds):
        dst = rng.integers(0, n, per_round).astype(np.uint32)
        pool = np.asarray([2, n // 2, n - 1, n + 7], np.uint32)  # (n + 7: outside the population, dead already)
        x = pool[rng.integers(0, pool.size, per_round)]  # four watchees at most: four slots never run out
        u = rng.random(per_round)
        tag = np.full(per_round, MIX_WATCH, np.uint32)
        tag[u < 0.55] = MIX_WITH
        tag[u < 0.30] = MIX_UNWATCH
        tag[u < 0.12] = MIX_STOP
        hit = (tag == MIX_STOP) & (rng.random(per_round) < 0.3)  # some stops go to a watchee of the pool
        dst[hit] = pool[rng.integers(0, 3, int(hit.sum()))]
        out.append((dst, (tag << np.uint32(24)) | x))
    return out


def snapshot(target, actors) -> dict:
    """everything the GPU tests compare bit for bit"""
    words, alive = target.read_state()
    info = target.watch_info()
    d, s, p = target.take_outbound()
    o = np.argsort(s, kind="stable")
    return dict(words=words.tolist(), alive=(alive & 1).tolist(), info=info,
                outbox=np.stack([s[o], d[o], p[o]]).tolist(),
                slots=[{k: v.tolist() for k, v in target.read_watch(a).items()} for a in actors])
