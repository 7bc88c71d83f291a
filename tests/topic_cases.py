"""The scenarios of the topic tests, shared by the CPU file (tests/test_topic_model.py: the model against the
reference spec's known answers, tests/golden/topic_kats.json, and the rules of DESIGN.md §2.10) and the GPU file
(tests/test_gpu_topics.py: the engine against the known answers and the model)."""
from __future__ import annotations

import json
import pathlib

import numpy as np

from akka_amd import typed
from akka_amd import workloads as wl

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "topic_kats.json").read_text())
TAGS, IDS, PUBLISHER = KATS["tags"], dict(KATS["ids"], P=KATS["publisher"]), KATS["publisher"]
SCENARIOS = {s["name"]: s for s in KATS["scenarios"]}
KAT_NAMES = tuple(SCENARIOS)
KAT_T = (1, 2, 5)
N_KAT = 64
NO_SENDER = 0xFFFFFFFF
COUNT_KEYS = ("delivered", "dead_letters", "unhandled", "emitted", "staged", "supersteps", "in_flight")
B = typed.Behaviors
ctx = typed.context
FRUIT, VEGGIES = typed.Topic("fruit"), typed.Topic("veggies")
MESH_SEEDS = (1, 2, 3)


def payload(msg: str) -> int:
    """'Name' or 'Name:arg' -> the u32 payload"""
    name, _, arg = msg.partition(":")
    return (TAGS[name] << 24) | int(arg or 0)


def _is(t):
    return lambda m: m.tag == TAGS[t]


def node_behavior(host: int) -> typed.Behavior:
    """Every actor of the scenarios.  Sub(k) / Unsub(k) subscribe to / unsubscribe from topic k (0 fruit, 1 veggies),
    Stop stops it; PubF(x) / PubV(x) publish Note(x) to fruit / veggies; SubPub(x) subscribes to fruit and publishes
    Note(x) there in one case, PubUnsub(x) publishes and unsubscribes; Count(k) answers the sender CountIs(subscriber
    count); a Note(x) is counted (state word 0), its sender -- the publisher -- kept (state word 1) and reported to the
    probe as Got(x); Ping(x) is reported as Got(x) too (so the probe sees the order of arrival); Poke(d) tells actor d
    Ping(d)."""
    st = typed.State("notes", "from_")
    probe = typed.actor_ref(host)
    note, ping = typed.MessageType("Note", TAGS["Note"]), typed.MessageType("Ping", TAGS["Ping"])
    rb = typed.ReceiveBuilder.create(st)
    rb.on_any_message(lambda m, s: [B.stopped], test=_is("Stop"))
    rb.on_any_message(lambda m, s: [s.notes.inc(), s.from_.set(m.sender.dst), probe.tell(m.arg, tag=TAGS["Got"]), B.same],
                      test=_is("Note"))
    rb.on_any_message(lambda m, s: [probe.tell(m.arg, tag=TAGS["Got"]), B.same], test=_is("Ping"))
    rb.on_any_message(lambda m, s: [typed.Ref(m.arg).tell(ping(m.arg)), B.same], test=_is("Poke"))
    rb.on_any_message(lambda m, s: [ctx.publish(FRUIT, note(m.arg)), B.same], test=_is("PubF"))
    rb.on_any_message(lambda m, s: [ctx.publish(VEGGIES, note(m.arg)), B.same], test=_is("PubV"))
    rb.on_any_message(lambda m, s: [ctx.subscribe(FRUIT), ctx.publish(FRUIT, note(m.arg)), B.same], test=_is("SubPub"))
    rb.on_any_message(lambda m, s: [ctx.publish(FRUIT, note(m.arg)), ctx.unsubscribe(FRUIT), B.same], test=_is("PubUnsub"))
    for k, tp in enumerate((FRUIT, VEGGIES)):
        arg = (lambda k: (lambda m, s: m.arg == k))(k)
        rb.on_any_message((lambda tp: lambda m, s: [ctx.subscribe(tp), B.same])(tp), test=_is("Sub"), when=arg)
        rb.on_any_message((lambda tp: lambda m, s: [ctx.unsubscribe(tp), B.same])(tp), test=_is("Unsub"), when=arg)
        rb.on_any_message((lambda tp: lambda m, s: [m.sender.tell(ctx.subscriber_count(tp), tag=TAGS["CountIs"]), B.same])(tp),
                          test=_is("Count"), when=arg)
    rb.on_any_message(lambda m, s: [B.unhandled])
    return rb.build("topic_node")


def node_workload(T: int, n: int = N_KAT, bucket_actors: int = 64, capacity: int = 0, log_capacity: int = 64, starts=(),
                  topics: bool = True) -> wl.Workload:
    """`n` actors running node_behavior, the probe at id n, topics fruit (0) and veggies (1); `starts`: (first, count,
    topic) subscribed in the setup block"""
    node = node_behavior(n)
    tb = typed.compile_behaviors([node], max_emit=1)
    assert tb.service_keys == [FRUIT, VEGGIES]
    return wl.Workload("topic_nodes", n, 2, 1, T, capacity, [(0, n, tb.kind_of(node), None)], behaviors=tb,
                       bucket_actors=bucket_actors, outbound=(n, 1),
                       receptionist={"n_keys": 2, "capacity": n, "starts": list(starts)},
                       topics={"log_capacity": log_capacity} if topics else {})


def target_host(target) -> int:
    return int(getattr(target, "n", None) or target.cfg.n_actors)


def tells(target, *msgs, src=None):
    """(dst, 'Name:arg') ... told from the probe"""
    dst = np.asarray([d for d, _ in msgs], np.uint32)
    pay = np.asarray([payload(m) for _, m in msgs], np.uint32)
    target.tell(dst, pay, np.full(dst.size, target_host(target) if src is None else src, np.uint32))


def counts(st) -> dict:
    return {k: (st[k] if isinstance(st, dict) else getattr(st, k)) for k in COUNT_KEYS}


def conserved(st, info) -> bool:
    return st["staged"] + st["emitted"] + info["fanned_out"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


def snapshot(t, n_keys: int = 2) -> dict:
    """everything the tests compare, from an engine or the model"""
    words, alive = t.read_state()
    d, s, p = t.take_outbound()
    o = np.argsort(s, kind="stable")  # per-sender order is the contract
    return dict(words=np.asarray(words).tolist(), alive=(np.asarray(alive) & 1).tolist(), info=t.receptionist_info(),
                topic_info=t.topic_info(), log=np.asarray(t.read_topic_log()).tolist(),
                listings=[t.read_listing(k).tolist() for k in range(n_keys)], masks=t.read_services().tolist(),
                outbox=np.stack([s[o], d[o], p[o]]).tolist(), kinds=np.asarray(t.read_kinds()).tolist())


def got_of(snap) -> dict:
    """actor -> the arguments of its Got reports, in order, from a snapshot's outbox"""
    out = {}
    for s, _, p in zip(*snap["outbox"]):
        if p >> 24 == TAGS["Got"]:
            out.setdefault(s, []).append(p & 0xFFFFFF)
    return out


# ------------------------------------------------------------------ the known answers
def run_kat(name: str, target) -> list:
    """run the scenario; per step what was observed: got, count, info"""
    out = []
    name_of = {v: k for k, v in IDS.items()}
    for step in SCENARIOS[name]["steps"]:
        tells(target, *[(IDS[a], m) for a, m in step["tell"]])
        target.run()
        d, s, p = target.take_outbound()
        g = {}
        if "got" in step:
            g["got"] = {}
            for ss, pp in zip(s.tolist(), p.tolist()):
                if pp >> 24 == TAGS["Got"]:
                    g["got"].setdefault(name_of[ss], []).append(pp & 0xFFFFFF)
        if "count" in step:
            g["count"] = [pp & 0xFFFFFF for pp in p.tolist() if pp >> 24 == TAGS["CountIs"]][0]
        if "info" in step:
            info = target.topic_info()
            g["info"] = {k: info[k] for k in step["info"]}
        out.append(g)
    return out


def check_kat(name: str, got: list) -> None:
    for i, (step, g) in enumerate(zip(SCENARIOS[name]["steps"], got)):
        for k, v in g.items():
            assert v == step[k], (name, i, k, v, step[k])


# ------------------------------------------------------------------ scripts: generators that yield every run's stats
def order_workload(T=5):
    """256 actors in four buckets of 64.  Fruit: 60..70 (straddles the boundary of buckets 0 and 1) and 200; veggies:
    62..66 and 201: the sets overlap in 62..66, and bucket 2 (128..191) has no subscriber"""
    return node_workload(T, n=256, starts=[(60, 11, 0), (200, 1, 0), (62, 5, 1), (201, 1, 1)])


def order_script(t):
    """publishers 5 (bucket 0), 130 (bucket 2) and 250 (bucket 3); 130 publishes twice in one window; subscriber 63
    also gets a device tell (from 7) and subscriber 64 a host-staged Ping in the tick of the delivery"""
    tells(t, (130, "PubF:1"), (5, "PubV:2"), (130, "PubV:3"), (250, "PubF:4"), (7, "Poke:63"))
    yield t.run(1)
    tells(t, (64, "Ping:9"), (63, "Ping:8"))
    yield t.run(1)
    yield t.run()


def timing_workload(T=3):
    return node_workload(T, n=256, starts=[(10, 1, 0), (70, 1, 0), (140, 1, 0), (141, 1, 0)])


def timing_script(t):
    """subscribe and publish in one tick from the same actor (20: receives) and from different actors (21 subscribes
    while 5 publishes: receives); publish then unsubscribe in one window (22: does not receive); unsubscribe in the tick
    of the publish (70: does not receive); a subscriber stopped in the tick of the publish (140: no delivery)"""
    tells(t, (22, "Sub:0"))
    yield t.run()
    tells(t, (20, "SubPub:1"), (21, "Sub:0"), (5, "PubF:2"), (22, "PubUnsub:3"), (70, "Unsub:0"), (140, "Stop"))
    yield t.run(1)
    yield t.run()
    # a subscriber stopped in the tick of the delivery, before draining it: a dead letter
    tells(t, (5, "PubF:4"))
    yield t.run(1)
    tells(t, (141, "Stop"))  # (the Stop is staged before the delivery in 141's inbox)
    yield t.run()
    # agx_register_services between the two ticks, both directions
    tells(t, (5, "PubF:5"))
    yield t.run(1)
    t.register_services(100, 3, 0, True)
    t.register_services(10, 1, 0, False)
    yield t.run()
    # a publication without a recipient waits for its tick; subscribers registered meanwhile receive it
    tells(t, (5, "PubV:6"))
    yield t.run()
    t.register_services(30, 2, 1, True)
    yield t.run()


def bounded_workload():
    return node_workload(1, n=128, capacity=2, starts=[(0, 128, 0)])


def bounded_script(t):
    """capacity 2, T = 1: three publications in one tick, every subscriber admits two and the third dies; the same
    again while every subscriber still holds one of them in its backlog"""
    tells(t, (1, "PubF:1"), (2, "PubF:2"), (3, "PubF:3"))
    yield t.run(2)
    tells(t, (4, "PubF:4"), (5, "PubF:5"), (6, "PubF:6"))
    yield t.run(2)
    yield t.run()


def budget_script(t):
    """run budgets that end between publish and delivery"""
    tells(t, (5, "PubF:1"), (6, "PubV:2"))
    yield t.run(1)
    yield t.run(1)
    tells(t, (5, "PubF:3"))
    yield t.run(1)
    tells(t, (7, "PubF:4"))
    yield t.run(1)
    yield t.run()


def host_publish_script(t):
    """agx_publish before the first run, between runs, after pending device publications, with no sender"""
    t.publish(0, payload("Note:1"), sender=300)
    t.publish(1, payload("Note:2"))
    yield t.run()
    tells(t, (5, "PubF:3"), (130, "PubF:4"))
    yield t.run(1)
    t.publish(0, payload("Note:5"), sender=NO_SENDER)
    t.publish(0, payload("Note:6"), sender=5)
    yield t.run(1)
    yield t.run()
    t.publish(1, payload("Note:7"), sender=301)
    yield t.run()


def mesh_workload(seed: int, bucket_actors: int) -> wl.Workload:
    return wl.topic_mesh(1024, 8, seed, 40, throughput=3, capacity=4, bucket_actors=bucket_actors)


def mesh_script(w):
    def script(t):
        for dst, src, pay in w.schedule:
            if len(dst):
                t.tell(dst, pay, src)
            yield t.run(1)
        yield t.run()
    return script
