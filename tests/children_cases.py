"""The scenarios of the children tests, shared by the CPU file (tests/test_children_model.py: the model against
WatchModel and the reference specs' known answers, tests/golden/children_kats.json) and the GPU file
(tests/test_gpu_children.py: the engine against the known answers and the model)."""
from __future__ import annotations

import json
import pathlib

import numpy as np

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.engine import NO_SENDER

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "children_kats.json").read_text())
TAGS, POOL_TAGS, ACTORS = KATS["tags"], KATS["pool_tags"], KATS["actors"]
SCENARIOS = {s["name"]: s for s in KATS["scenarios"]}
KAT_NAMES = tuple(SCENARIOS)
KAT_T = (1, 3)
N_KAT, HOST = 64, 64
COUNT_KEYS = ("delivered", "dead_letters", "unhandled", "emitted", "staged", "supersteps", "in_flight")
CHILD_KEYS = ("spawned", "refused", "created", "child_stops", "cascade_stops", "illegal_stops", "discarded", "live")
NONE = 0xFFFFFFFF
B = typed.Behaviors
ctx = typed.context


def payload(msg: str, tags=TAGS) -> int:
    """'Name' or 'Name:arg' -> the u32 payload"""
    name, _, arg = msg.partition(":")
    return (tags[name] << 24) | int(arg or 0)


def _is(t):
    return lambda m: m.tag == TAGS[t]


def child_behavior(host: int = HOST) -> typed.Behavior:
    """Stop stops it; Work is counted and echoed to the monitor; its state: (count, the parent's id)."""
    return (typed.ReceiveBuilder.create(typed.State("n", "parent"))
            .on_any_message(lambda m, s: [B.stopped], test=_is("Stop"))
            .on_any_message(lambda m, s: [s.n.inc(), typed.actor_ref(host).tell(m.payload), B.same], test=_is("Work"))
            .on_any_message(lambda m, s: [B.unhandled]).build("child"))


def parent_behavior(child: typed.Behavior, host: int = HOST) -> typed.Behavior:
    """The parent of the ActorContextSpec scenarios, driven by messages: Spawn(arg) spawns a child (its id goes
    into `child`), SpawnWatch spawns and watches it in one case, StopChild is context.stop(the last child),
    StopRef(x) context.stop(x), Watch(x) / Unwatch(x), Stop stops it; Terminated(ref) is counted and echoed as
    Got(ref)."""
    hostr = typed.actor_ref(host)
    st = typed.State("child", "seen")
    ref = lambda m: typed.Ref(m.arg)
    spawn = lambda m, s: ctx.spawn(child, arg=m.arg, word1=ctx.PARENT, into=s.child)
    return (typed.ReceiveBuilder.create(st)
            .on_any_message(lambda m, s: [spawn(m, s), B.same], test=_is("Spawn"))
            .on_any_message(lambda m, s: [spawn(m, s), ctx.watch(s.child.ref), B.same], test=_is("SpawnWatch"))
            .on_any_message(lambda m, s: [ctx.stop(s.child.ref), B.same], test=_is("StopChild"))
            .on_any_message(lambda m, s: [ctx.stop(ref(m)), s.seen.add(100), B.same], test=_is("StopRef"))
            .on_any_message(lambda m, s: [ctx.watch(ref(m)), B.same], test=_is("Watch"))
            .on_any_message(lambda m, s: [ctx.unwatch(ref(m)), B.same], test=_is("Unwatch"))
            .on_any_message(lambda m, s: [B.stopped], test=_is("Stop"))
            .on_any_message(lambda m, s: [B.unhandled])
            .on_signal(typed.Terminated, lambda sig, s: [s.seen.inc(), hostr.tell(sig.ref.dst, tag=TAGS["Got"]), B.same])
            .build("parent"))


def parent_workload(T: int, n: int = N_KAT, parents=(0, 8), first_child: int = 40, max_children: int = 4,
                    bucket_actors: int = 32, n_slots: int = 2, capacity: int = 0, extra_regions=()) -> wl.Workload:
    """actors `parents` = (first, count) run the parent behaviour (their children: `max_children` ids each from
    `first_child`); every child-block id starts unregistered"""
    child = child_behavior(n)
    par = parent_behavior(child, n)
    tb = typed.compile_behaviors([par, child], max_emit=1)
    regions = [(parents[0], parents[1], first_child, max_children)] + list(extra_regions)
    return wl.Workload("children", n, 2, 1, T, capacity, [(parents[0], parents[1], tb.kind_of(par), None)], behaviors=tb,
                       outbound=(n, 1), bucket_actors=bucket_actors, watch={"n_slots": n_slots},
                       children={"regions": regions, "sites": tb.spawn_sites})


def kat_workload(name: str, T: int) -> wl.Workload:
    if SCENARIOS[name]["setup"] == "pool":
        w = wl.pool_router(1, 4, throughput=T, bucket_actors=32, host_id=HOST)
        w.n_actors = N_KAT  # (ids 5..63 stay unregistered)
        return w
    # parent 2 of the JSON is the first parent: its children are 40..43; the bystander 5 is a parent too
    return parent_workload(T, parents=(2, 4), first_child=40, max_children=4)


def counts(st) -> dict:
    return {k: (st[k] if isinstance(st, dict) else getattr(st, k)) for k in COUNT_KEYS}


def per_sender(target):
    d, s, p = target.take_outbound()
    o = np.argsort(s, kind="stable")
    return [[int(a), int(x)] for a, x in zip(s[o], p[o])]


def run_kat(name: str, T: int, target) -> dict:
    sc = SCENARIOS[name]
    tags = POOL_TAGS if sc["setup"] == "pool" else TAGS
    echo, st = [], None
    for step in sc["script"]:
        if step["tell"]:
            d = np.asarray([ACTORS[a] for a, _ in step["tell"]], np.uint32)
            p = np.asarray([payload(m, tags) for _, m in step["tell"]], np.uint32)
            target.tell(d, p, np.full(p.size, NO_SENDER, np.uint32))
        st = counts(target.run())
        echo.append(per_sender(target))
    _, alive = target.read_state()
    return dict(echo=echo, counts=st, info=target.children_info(), terminated=target.watch_info()["terminated"],
                alive={a: int(alive[ACTORS[a]] & 1) for a in sc["final"]["alive"]})


def check_kat(name: str, T: int, got: dict) -> None:
    """`got` against the JSON."""
    sc = SCENARIOS[name]
    tags = POOL_TAGS if sc["setup"] == "pool" else TAGS
    assert got["echo"] == [[[ACTORS[a], payload(m, tags)] for a, m in e] for e in sc["echo"]], (got["echo"], sc["echo"])
    assert got["info"] == sc["final"]["info"], got["info"]
    assert got["alive"] == sc["final"]["alive"], got["alive"]
    c = got["counts"]
    assert c["in_flight"] == 0
    assert c["staged"] + c["emitted"] + got["terminated"] == c["delivered"] + c["dead_letters"] + c["in_flight"]


def tells(target, *msgs, src=NO_SENDER):
    """(dst, 'Name[:arg]') ..."""
    d = np.asarray([m[0] for m in msgs], np.uint32)
    p = np.asarray([payload(m[1]) for m in msgs], np.uint32)
    target.tell(d, p, np.full(d.size, src, np.uint32))


def snapshot(target, actors) -> dict:
    """everything the GPU tests compare bit for bit"""
    words, alive = target.read_state()
    return dict(words=words.tolist(), alive=(alive & 1).tolist(), watch=target.watch_info(), children=target.children_info(),
                outbox=per_sender(target),
                slots=[{k: v.tolist() for k, v in target.read_watch(a).items()} for a in actors],
                kids=[target.read_children(a) for a in actors])
