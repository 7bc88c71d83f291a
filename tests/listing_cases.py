"""The scenarios of the Subscribe / Listing tests, shared by the CPU file (tests/test_listing_model.py: the model against
the reference spec's known answers, tests/golden/listing_kats.json, and the rules of DESIGN.md §2.11) and the GPU files
(tests/test_gpu_listings.py: the engine against the known answers and the model)."""
from __future__ import annotations

import json
import pathlib

import numpy as np

from akka_amd import typed
from akka_amd import workloads as wl

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "listing_kats.json").read_text())
TAGS, IDS = KATS["tags"], KATS["ids"]
SCENARIOS = {s["name"]: s for s in KATS["scenarios"]}
KAT_NAMES = tuple(SCENARIOS)
KAT_T = (1, 5)
N_KAT = 64
NO_SENDER = 0xFFFFFFFF
COUNT_KEYS = ("delivered", "dead_letters", "unhandled", "emitted", "staged", "supersteps", "in_flight")
B = typed.Behaviors
ctx = typed.context
KEY_A, KEY_B = typed.ServiceKey("ServiceKeyA"), typed.ServiceKey("ServiceKeyB")
FRUIT = typed.Topic("fruit")
KEYS = (KEY_A, KEY_B)
LISTING = (typed.MessageType("ListingA", TAGS["LstA"]), typed.MessageType("ListingB", TAGS["LstB"]))
N_KEYS = 3  # ServiceKeyA, ServiceKeyB and the topic
MESH_SEEDS = (1, 2, 3)


def payload(msg: str) -> int:
    """'Name' or 'Name:arg' -> the u32 payload"""
    name, _, arg = msg.partition(":")
    return (TAGS[name] << 24) | int(arg or 0)


def _is(t):
    return lambda m: m.tag == TAGS[t]


def node_behavior(host: int) -> typed.Behavior:
    """Every actor of the scenarios.  Sub(k) / Find(k) subscribe to / find key k (0 ServiceKeyA, 1 ServiceKeyB), Reg(k)
    / Dereg(k) register / deregister the actor under it, RegDereg(k) does both in one case, Stop stops it.  A Listing
    of key k is counted (state word 0), the first id of the listing in force kept (state word 1) and its size reported
    to the probe under the key's own tag (LstA / LstB).  TSub subscribes to the topic fruit, Pub(x) publishes Note(x)
    there; a Note(x) and a Ping(x) are reported as Got(x) (so the probe sees the order of arrival); Poke(d) tells actor
    d Ping(d)."""
    st = typed.State("listings", "first")
    probe = typed.actor_ref(host)
    note, ping = typed.MessageType("Note", TAGS["Note"]), typed.MessageType("Ping", TAGS["Ping"])
    rb = typed.ReceiveBuilder.create(st)
    rb.on_any_message(lambda m, s: [B.stopped], test=_is("Stop"))
    for k, key in enumerate(KEYS):
        rb.on_message(LISTING[k], (lambda k, key: lambda m, s: [s.listings.inc(), s.first.set(ctx.service_at(key, 0).dst),
                                                                probe.tell(ctx.listing_size(key), tag=LISTING[k].tag), B.same])(k, key))
    rb.on_any_message(lambda m, s: [probe.tell(m.arg, tag=TAGS["Got"]), B.same], test=_is("Note"))
    rb.on_any_message(lambda m, s: [probe.tell(m.arg, tag=TAGS["Got"]), B.same], test=_is("Ping"))
    rb.on_any_message(lambda m, s: [typed.Ref(m.arg).tell(ping(m.arg)), B.same], test=_is("Poke"))
    rb.on_any_message(lambda m, s: [ctx.subscribe(FRUIT), B.same], test=_is("TSub"))
    rb.on_any_message(lambda m, s: [ctx.publish(FRUIT, note(m.arg)), B.same], test=_is("Pub"))
    for k, key in enumerate(KEYS):
        arg = (lambda k: (lambda m, s: m.arg == k))(k)
        rb.on_any_message((lambda k, key: lambda m, s: [ctx.receptionist_subscribe(key, LISTING[k]), B.same])(k, key),
                          test=_is("Sub"), when=arg)
        rb.on_any_message((lambda k, key: lambda m, s: [ctx.receptionist_find(key, LISTING[k]), B.same])(k, key),
                          test=_is("Find"), when=arg)
        rb.on_any_message((lambda key: lambda m, s: [ctx.register(key), B.same])(key), test=_is("Reg"), when=arg)
        rb.on_any_message((lambda key: lambda m, s: [ctx.deregister(key), B.same])(key), test=_is("Dereg"), when=arg)
        rb.on_any_message((lambda key: lambda m, s: [ctx.register(key), ctx.deregister(key), B.same])(key),
                          test=_is("RegDereg"), when=arg)
    rb.on_any_message(lambda m, s: [B.unhandled])
    return rb.build("listing_node")


def node_tables(host: int):
    node = node_behavior(host)
    tb = typed.compile_behaviors([node], max_emit=1)
    assert tb.service_keys == [KEY_A, KEY_B, FRUIT]
    return node, tb


def node_workload(T: int, n: int = N_KAT, bucket_actors: int = 64, capacity: int = 0, registered=(), subscribed=(),
                  listings: bool = True, topics: bool = True) -> wl.Workload:
    """`n` actors running node_behavior, the probe at id n; `registered` / `subscribed`: (first, count, key) of the
    setup block (agx_register_services / agx_subscribe_listings)"""
    node, tb = node_tables(n)
    return wl.Workload("listing_nodes", n, 2, 1, T, capacity, [(0, n, tb.kind_of(node), None)], behaviors=tb,
                       bucket_actors=bucket_actors, outbound=(n, 1),
                       receptionist={"n_keys": N_KEYS, "capacity": n, "starts": list(registered)},
                       topics={"log_capacity": 16} if topics else {},
                       listings={"payloads": tb.listing_payloads, "starts": list(subscribed)} if listings else {})


def target_host(target) -> int:
    return int(getattr(target, "n", None) or target.cfg.n_actors)


def tells(target, *msgs, src=None):
    """(dst, 'Name:arg') ... told from the probe"""
    dst = np.asarray([d for d, _ in msgs], np.uint32)
    pay = np.asarray([payload(m) for _, m in msgs], np.uint32)
    target.tell(dst, pay, np.full(dst.size, target_host(target) if src is None else src, np.uint32))


def counts(st) -> dict:
    return {k: (st[k] if isinstance(st, dict) else getattr(st, k)) for k in COUNT_KEYS}


def conserved(st, topic_info, listing_info) -> bool:
    return (st["staged"] + st["emitted"] + topic_info["fanned_out"] + listing_info["listings_sent"]
            == st["delivered"] + st["dead_letters"] + st["in_flight"])


def snapshot(t, n_keys: int = N_KEYS) -> dict:
    """everything the tests compare, from an engine or the model"""
    words, alive = t.read_state()
    d, s, p = t.take_outbound()
    o = np.argsort(s, kind="stable")  # per-sender order is the contract
    sub, pend = t.read_subscriptions()
    return dict(words=np.asarray(words).tolist(), alive=(np.asarray(alive) & 1).tolist(), info=t.receptionist_info(),
                topic_info=t.topic_info(), listing_info=t.listing_info(), log=np.asarray(t.read_topic_log()).tolist(),
                listings=[t.read_listing(k).tolist() for k in range(n_keys)], masks=t.read_services().tolist(),
                sub=np.asarray(sub).tolist(), pending=np.asarray(pend).tolist(),
                outbox=np.stack([s[o], d[o], p[o]]).tolist(), kinds=np.asarray(t.read_kinds()).tolist())


def reports_of(snap) -> dict:
    """actor -> what it reported to the probe, in order, from a snapshot's outbox: ('L', key, size) per Listing,
    ('G', x) per Note or Ping"""
    out = {}
    for s, _, p in zip(*snap["outbox"]):
        tag = p >> 24
        if tag == TAGS["Got"]:
            out.setdefault(s, []).append(("G", p & 0xFFFFFF))
        elif tag in (TAGS["LstA"], TAGS["LstB"]):
            out.setdefault(s, []).append(("L", tag - TAGS["LstA"], p & 0xFFFFFF))
    return out


# ------------------------------------------------------------------ the known answers
def run_kat(name: str, target) -> list:
    """run the scenario; per step what was observed: got, listing, info"""
    out = []
    name_of = {v: k for k, v in IDS.items()}
    for step in SCENARIOS[name]["steps"]:
        tells(target, *[(IDS[a], m) for a, m in step["tell"]])
        target.run()
        d, s, p = target.take_outbound()
        g = {"got": {}}
        for ss, pp in zip(s.tolist(), p.tolist()):
            if pp >> 24 in (TAGS["LstA"], TAGS["LstB"]):
                g["got"].setdefault(name_of[ss], []).append([(pp >> 24) - TAGS["LstA"], pp & 0xFFFFFF])
        if "listing" in step:
            g["listing"] = {k: [name_of[a] for a in target.read_listing(int(k)).tolist()] for k in step["listing"]}
        if "info" in step:
            info = target.listing_info()
            g["info"] = {k: info[k] for k in step["info"]}
        out.append(g)
    return out


def check_kat(name: str, got: list) -> None:
    steps = SCENARIOS[name]["steps"]
    assert len(got) == len(steps)
    for i, (step, g) in enumerate(zip(steps, got)):
        for k, v in g.items():
            assert v == step.get(k, {}), (name, i, k, v, step.get(k))
        for sub, ls in g["got"].items():  # a Listing's size is the size of the set the spec expects
            for key, size in ls:
                if "listing" in step and str(key) in step["listing"]:
                    assert size == len(step["listing"][str(key)]), (name, i, sub, key, size)


# ------------------------------------------------------------------ scripts: generators that yield every run's stats
def order_workload(T=5):
    """250 actors in buckets of 64: the last bucket (192..249) holds 58.  Subscribers of key A on both sides of every
    bucket boundary (63, 64, 127, 128, 191, 192) and at the end of the short bucket (249); of key B: 63, 64, 200; 64
    and 200 also subscribe to the topic; services: 5 under A, 6 under B"""
    return node_workload(T, n=250, registered=[(5, 1, 0), (6, 1, 1), (64, 1, 2), (200, 1, 2)],
                         subscribed=[(63, 2, 0), (127, 2, 0), (191, 2, 0), (249, 1, 0), (63, 2, 1), (200, 1, 1)])


def order_script(t):
    """the initial Listings; then two keys change in one tick (7 registers under A, 6 deregisters under B) while 130
    publishes to the topic and 3 pokes 64: subscriber 64 receives its Ping (an arrival), a host-staged Ping, the
    publication and its two Listings in that order, A before B"""
    yield t.run()
    tells(t, (7, "Reg:0"), (6, "Dereg:1"), (130, "Pub:9"), (3, "Poke:64"))
    yield t.run(1)
    tells(t, (64, "Ping:8"))
    yield t.run(1)
    yield t.run()


def backlog_script(t):
    """T = 1: subscriber 64 holds two Pings when key A changes: the Listing queues behind them, and the handler sees
    the listing in force when it is drained"""
    yield t.run()
    tells(t, (64, "Ping:1"), (64, "Ping:2"), (64, "Ping:3"), (7, "Reg:0"))
    yield t.run(1)
    tells(t, (8, "Reg:0"))  # (a second change while the first Listing still waits)
    yield t.run(1)
    yield t.run(1)
    yield t.run()


def timing_workload(T=3):
    return node_workload(T, n=256, registered=[(5, 1, 0)], subscribed=[(70, 1, 0), (140, 1, 0), (141, 1, 0)])


def timing_script(t):
    """Subscribe in tick s with a change in s (20 subscribes while 6 registers: one Listing) and without (21, key B:
    one Listing); Find by a non-subscriber (22: one Listing, none later); Find by a subscriber whose key also changed
    (70: one envelope); register then deregister in one window (7: no version move, nobody is told); a registered
    actor's stop notifies (5); a subscriber stopped in the tick of a change gets nothing (140); subscribe and stop in
    one window (23) gives no Listing"""
    yield t.run()
    tells(t, (20, "Sub:0"), (6, "Reg:0"), (21, "Sub:1"), (22, "Find:0"), (70, "Find:0"))
    yield t.run(1)
    yield t.run()
    tells(t, (7, "RegDereg:0"))
    yield t.run()
    tells(t, (8, "Reg:1"), (8, "Dereg:1"))  # (two messages of one window: T = 3)
    yield t.run()
    tells(t, (5, "Stop"), (140, "Stop"), (23, "Sub:0"), (23, "Stop"))
    yield t.run(1)
    yield t.run()
    tells(t, (20, "Sub:0"))  # a repeated Subscribe: the immediate reply again
    yield t.run()


def bounded_workload():
    return node_workload(1, n=130, capacity=2, subscribed=[(0, 128, 0), (0, 128, 1)])


def bounded_script(t):
    """capacity 2, T = 1: the two initial Listings fill every subscriber's mailbox in tick 1, in which both keys
    change (128 and 129 register); in tick 2 every subscriber still holds its initial Listing of B: the new Listing of
    A is admitted, the new Listing of B is a dead letter (by position)"""
    tells(t, (128, "Reg:0"), (129, "Reg:1"))
    yield t.run(1)
    yield t.run(1)
    yield t.run()


def budget_script(t):
    """run budgets that end between a change and its Listings"""
    tells(t, (7, "Reg:0"))
    yield t.run(1)
    yield t.run(1)
    yield t.run()
    yield t.run()


def host_calls_script(t):
    """agx_subscribe_listings gives its initial Listings; agx_register_services that changes a bit notifies every
    subscriber exactly once, also after a run whose last tick changed that key; one that changes nothing notifies
    nobody; several calls, and calls for two keys, between two runs"""
    yield t.run()
    t.subscribe_listings(100, 3, 0, True)
    t.subscribe_listings(63, 1, 0, False)  # (63 no longer subscribes to A)
    yield t.run()
    t.register_services(9, 2, 0, True)
    yield t.run()
    t.register_services(9, 2, 0, True)  # (changes nothing)
    yield t.run()
    tells(t, (11, "Reg:0"))
    yield t.run(1)  # (the run's last tick changed key A: its Listings are owed ...)
    t.register_services(12, 1, 0, True)  # (... and the host changes it again: one Listing each)
    yield t.run()
    t.register_services(13, 1, 0, True)
    t.register_services(13, 1, 1, True)
    t.register_services(14, 1, 0, True)
    t.publish(2, payload("Note:5"))  # (a re-plan without another rebuild in between)
    yield t.run(1)
    yield t.run()
    tells(t, (15, "Reg:1"))
    yield t.run(1)
    t.publish(2, payload("Note:6"))  # (no register call: the change of the last tick is not counted twice)
    yield t.run()


def tile_workload():
    """one 2048-actor bucket, every actor subscribed to key A in the setup block"""
    return node_workload(3, n=2048, bucket_actors=2048, subscribed=[(0, 2048, 0)])


def tile_script(keys_changing: int):
    """every actor subscribes to both keys (key B between two runs: each set of 2048 initial Listings is exactly one
    tile); then `keys_changing` of them change in one tick"""
    def script(t):
        yield t.run()
        t.subscribe_listings(0, 2048, 1, True)
        yield t.run()
        tells(t, *[(5, "Reg:0"), (6, "Reg:1")][:keys_changing])
        yield t.run()
    return script


def mesh_workload(seed: int, n: int, bucket_actors: int) -> wl.Workload:
    """the seeded random mesh: per tick a few random actors subscribe, find, register, deregister, stop, subscribe to
    the topic or publish"""
    rng = np.random.default_rng(seed)
    w = node_workload(3, n=n, bucket_actors=bucket_actors, capacity=6, registered=[(int(rng.integers(0, n - 8)), 8, 0)],
                      subscribed=[(int(rng.integers(0, n - 16)), 16, 1)])
    per = {"Sub": max(n // 64, 1), "Find": max(n // 128, 1), "Reg": max(n // 128, 1), "Dereg": max(n // 128, 1),
           "Stop": max(n // 256, 1), "RegDereg": 1, "TSub": max(n // 128, 1), "Pub": 1, "Poke": 2}
    schedule = []
    for tick in range(24):
        dst, pay = [], []
        for name, cnt in per.items():
            if tick % 3 == 2 and name in ("Reg", "Dereg", "Stop", "RegDereg"):  # (some ticks change no key)
                continue
            d = rng.integers(0, n, cnt)
            arg = d if name == "Poke" else rng.integers(0, 2, cnt) if name != "Pub" else rng.integers(0, 100, cnt)
            dst.append(d if name != "Poke" else rng.integers(0, n, cnt))
            pay.append((TAGS[name] << 24) | arg)
        dst = np.concatenate(dst).astype(np.uint32)
        o = rng.permutation(dst.size)
        schedule.append((dst[o], np.full(dst.size, n, np.uint32), np.concatenate(pay).astype(np.uint32)[o]))
    w.schedule = schedule
    return w


def mesh_script(w):
    def script(t):
        for dst, src, pay in w.schedule:
            if len(dst):
                t.tell(dst, pay, src)
            yield t.run(1)
        yield t.run()
    return script
