"""The scenarios of the receptionist tests, shared by the CPU file (tests/test_receptionist_model.py: the model
against the reference specs' known answers, tests/golden/receptionist_kats.json) and the GPU file
(tests/test_gpu_receptionist.py: the engine against the known answers and the model)."""
from __future__ import annotations

import json
import pathlib

import numpy as np

from akka_amd import typed
from akka_amd import workloads as wl

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "receptionist_kats.json").read_text())
TAGS, IDS, ROUTER = KATS["tags"], KATS["ids"], KATS["router"]
SCENARIOS = {s["name"]: s for s in KATS["scenarios"]}
KAT_NAMES = tuple(SCENARIOS)
KAT_T = (1, 3)
N_KAT = 64
COUNT_KEYS = ("delivered", "dead_letters", "unhandled", "emitted", "staged", "supersteps", "in_flight")
B = typed.Behaviors
ctx = typed.context
KEYS = [typed.ServiceKey("svc0"), typed.ServiceKey("svc1")]


def payload(msg: str) -> int:
    """'Name' or 'Name:arg' -> the u32 payload"""
    name, _, arg = msg.partition(":")
    return (TAGS[name] << 24) | int(arg or 0)


def _is(t):
    return lambda m: m.tag == TAGS[t]


def node_behavior(keys=KEYS) -> typed.Behavior:
    """Every actor of the scenarios: Reg(k) / Dereg(k) register under / deregister from key k, Stop stops it;
    Route(x) routes Work(x) round robin over key 0 (cursor: state word 0) as a forward, RouteBy(x) by index x; Size(k)
    answers the sender SizeIs(listing size), At(x) answers AtIs(listing[x mod size]) of key 0 (Find, read
    synchronously); Work(x) is counted (state word 1) and answered to its sender -- the forward's replyTo -- as Did(x)."""
    st = typed.State("cursor", "done")
    rb = typed.ReceiveBuilder.create(st)
    rb.on_any_message(lambda m, s: [B.stopped], test=_is("Stop"))
    rb.on_any_message(lambda m, s: [s.done.inc(), m.sender.tell(m.arg, tag=TAGS["Did"]), B.same], test=_is("Work"))
    work = typed.MessageType("Work", TAGS["Work"])
    rb.on_any_message(lambda m, s: [ctx.route(keys[0], work(m.arg), cursor=s.cursor), B.same], test=_is("Route"))
    rb.on_any_message(lambda m, s: [ctx.route_by(keys[0], m.arg, work(m.arg)), B.same], test=_is("RouteBy"))
    rb.on_any_message(lambda m, s: [m.sender.tell(ctx.service_at(keys[0], m.arg).dst, tag=TAGS["AtIs"]), B.same], test=_is("At"))
    for k, key in enumerate(keys):
        arg = (lambda k: (lambda m, s: m.arg == k))(k)
        rb.on_any_message((lambda key: lambda m, s: [ctx.register(key), B.same])(key), test=_is("Reg"), when=arg)
        rb.on_any_message((lambda key: lambda m, s: [ctx.deregister(key), B.same])(key), test=_is("Dereg"), when=arg)
        rb.on_any_message((lambda key: lambda m, s: [m.sender.tell(ctx.listing_size(key), tag=TAGS["SizeIs"]), B.same])(key),
                          test=_is("Size"), when=arg)
    rb.on_any_message(lambda m, s: [B.unhandled])
    return rb.build("svc_node")


def node_workload(T: int, n: int = N_KAT, bucket_actors: int = 64, capacity: int = 0, n_keys: int = 2, listing_capacity=None,
                  starts=(), host=None) -> wl.Workload:
    """`n` actors running node_behavior, the probe at id `host` (default n), `n_keys` service keys"""
    keys = [typed.ServiceKey(f"svc{k}") for k in range(n_keys)]
    node = node_behavior(keys)
    tb = typed.compile_behaviors([node], max_emit=1)
    host = n if host is None else host
    return wl.Workload("svc_nodes", n, 2, 1, T, capacity, [(0, n, tb.kind_of(node), None)], behaviors=tb,
                       bucket_actors=bucket_actors, outbound=(host, 1),
                       receptionist={"n_keys": n_keys, "capacity": n if listing_capacity is None else listing_capacity,
                                     "starts": list(starts)})


def tells(target, *msgs, src=None):
    """(dst, 'Name:arg') ... told from the probe"""
    dst = np.asarray([d for d, _ in msgs], np.uint32)
    pay = np.asarray([payload(m) for _, m in msgs], np.uint32)
    target.tell(dst, pay, np.full(dst.size, target_host(target) if src is None else src, np.uint32))


def target_host(target) -> int:
    return int(getattr(target, "n", None) or target.cfg.n_actors)


def counts(st) -> dict:
    return {k: (st[k] if isinstance(st, dict) else getattr(st, k)) for k in COUNT_KEYS}


def snapshot(t, n_keys: int) -> dict:
    """everything the tests compare, from an engine or the model"""
    words, alive = t.read_state()
    d, s, p = t.take_outbound()
    o = np.argsort(s, kind="stable")  # per-sender order is the contract
    return dict(words=np.asarray(words).tolist(), alive=(np.asarray(alive) & 1).tolist(), info=t.receptionist_info(),
                listings=[t.read_listing(k).tolist() for k in range(n_keys)], masks=t.read_services().tolist(),
                outbox=np.stack([s[o], d[o], p[o]]).tolist(), kinds=np.asarray(t.read_kinds()).tolist())


# ------------------------------------------------------------------ the known answers
def kat_workload(name: str, T: int) -> wl.Workload:
    sc = SCENARIOS[name]
    return node_workload(T, starts=[(IDS[x], 1, 0) for x in sc["setup"]])


def run_kat(name: str, T: int, target) -> list:
    """run the scenario; per step what was observed: picks, listing, listing1, find, masks, info, version0"""
    sc, out = SCENARIOS[name], []
    name_of = {v: k for k, v in IDS.items()}
    for step in sc["steps"]:
        got = {}
        if "tell" in step:
            tells(target, *[(IDS[a], m) for a, m in step["tell"]])
            target.run()
        if "route" in step:
            tells(target, *[(ROUTER, f"Route:{i}") for i in range(step["route"])])
            target.run()
            d, s, p = target.take_outbound()
            who = {int(pp) & 0xFFFFFF: int(ss) for dd, ss, pp in zip(d, s, p) if int(pp) >> 24 == TAGS["Did"]}
            got["picks"] = [name_of.get(who.get(i)) for i in range(step["route"])]
        if "find" in step:
            tells(target, (ROUTER, "Size:0"), (ROUTER, "At:0"))
            target.run()
            d, s, p = target.take_outbound()
            by = {int(pp) >> 24: int(pp) & 0xFFFFFF for pp in p}
            got["find"] = {"size": by[TAGS["SizeIs"]], "at0": name_of.get(by[TAGS["AtIs"]])}
        info = target.receptionist_info()
        if "listing" in step:
            got["listing"] = [name_of[int(x)] for x in target.read_listing(0)]
        if "listing1" in step:
            got["listing1"] = [name_of[int(x)] for x in target.read_listing(1)]
        if "masks" in step:
            m = target.read_services()
            got["masks"] = {a: int(m[IDS[a]]) for a in step["masks"]}
        if "info" in step:
            got["info"] = {k: info[k] for k in step["info"]}
        if "version0" in step:
            got["version0"] = info["version"][0]
        out.append(got)
    return out


def check_kat(name: str, got: list) -> None:
    for i, (step, g) in enumerate(zip(SCENARIOS[name]["steps"], got)):
        for k, v in g.items():
            assert v == step[k], (name, i, k, v, step[k])
