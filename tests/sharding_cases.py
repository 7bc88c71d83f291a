"""The scenarios of the sharding tests, shared by the CPU file (tests/test_sharding_model.py: the model against the
known answers) and the GPU file (tests/test_gpu_sharding.py: the engine against the known answers and the model).
Populations of 80 ids in buckets of 32 (a partial last bucket): registered plain actors 0..19 and 70..79, entity type
`counter` = ids 20..43 (it straddles the bucket boundary at 32), entity type `idle` = ids 50..69 (it straddles the one
at 64; receive timeout 3).  The known answers (tests/golden/sharding_kats.json) are worked out by hand from
akka-cluster-sharding's Shard.scala: no JVM is available to record them."""
from __future__ import annotations

import json
import pathlib

import numpy as np

from akka_amd import typed
from akka_amd import workloads as wl
from akka_amd.engine import NO_SENDER
from tests.prio_model import per_sender

KATS = json.loads((pathlib.Path(__file__).parent / "golden" / "sharding_kats.json").read_text())
TAGS = KATS["tags"]
SCENARIOS = {s["name"]: s for s in KATS["scenarios"]}
KAT_NAMES = tuple(SCENARIOS)
KAT_T = (1, 2, 16)
N_KAT, HOST = 80, 80
PLAIN = ((0, 20), (70, 10))
COUNTER, IDLE = (20, 24), (50, 20)
IDLE_DELAY = 3
COUNT_KEYS = ("delivered", "dead_letters", "unhandled", "emitted", "staged", "supersteps", "in_flight")
SHARD_KEYS = ("started", "restarted", "passivations", "passivated", "passivate_ignored", "passivate_unknown", "alive")
B = typed.Behaviors


def payload(msg: str) -> int:
    """'Name' or 'Name:arg' -> the u32 payload"""
    name, _, arg = msg.partition(":")
    return (TAGS[name] << 24) | int(arg or 0)


def mtype(name: str) -> typed.MessageType:
    return typed.MessageType(name, TAGS[name])


def behaviors():
    """The entity: Job (and TimerJob, what Arm's timer delivers) is counted in word 0 -- the jobs of this incarnation --
    and answered with Done:<count> to the host; Passivate and Idle (the idle type's receive timeout) passivate; Bye is
    the stop message; Stop is a plain stop; SelfTell sends itself a Job, SelfStop does so and stops; Arm starts a
    single timer of 1 tick.  The plain actor: Fwd:<id> sends a Job to that id, Passivate passivates (it is no entity),
    Job is counted, Stop stops."""
    host = typed.actor_ref(HOST)
    st = typed.State("jobs", "id")
    ctx = typed.context

    def build(timers):
        timers.cancel("t")
        counted = lambda m, s: [s.jobs.inc(), host.tell(mtype("Done")(s.jobs)), B.same]
        return (typed.ReceiveBuilder.create(st)
                .on_message(mtype("Job"), counted)
                .on_message(mtype("TimerJob"), counted)
                .on_message(mtype("Passivate"), lambda m, s: [ctx.passivate(), B.same])
                .on_message(mtype("Idle"), lambda m, s: [ctx.passivate(), B.same])
                .on_message(mtype("Bye"), lambda m, s: [B.stopped])
                .on_message(mtype("Stop"), lambda m, s: [B.stopped])
                .on_message(mtype("SelfTell"), lambda m, s: [typed.self_ref().tell(mtype("Job")()), B.same])
                .on_message(mtype("SelfStop"), lambda m, s: [typed.self_ref().tell(mtype("Job")()), B.stopped])
                .on_message(mtype("Arm"), lambda m, s: [timers.start_single_timer("t", mtype("TimerJob")(), 1), B.same])
                .on_any_message(lambda m, s: [B.unhandled])
                .build("entity"))
    entity = B.with_timers(build)
    ps = typed.State("count", "unused")
    plain = (typed.ReceiveBuilder.create(ps)
             .on_message(mtype("Fwd"), lambda m, s: [typed.Ref(m.arg).tell(mtype("Job")()), B.same])
             .on_message(mtype("Passivate"), lambda m, s: [ctx.passivate(), B.same])
             .on_message(mtype("Job"), lambda m, s: [s.count.inc(), B.same])
             .on_message(mtype("Stop"), lambda m, s: [B.stopped])
             .on_any_message(lambda m, s: [B.unhandled])
             .build("plain"))
    return entity, plain


def entities(entity):
    key = typed.EntityTypeKey
    return [typed.Entity(key("counter"), entity, *COUNTER, word1=typed.Entity.ID).with_stop_message(mtype("Bye")()),
            typed.Entity(key("idle"), entity, *IDLE, word1=typed.Entity.ID).with_stop_message(mtype("Bye")())
            .with_receive_timeout(IDLE_DELAY, mtype("Idle")())]


def kat_workload(T: int, capacity: int = 0, sharding: bool = True) -> wl.Workload:
    entity, plain = behaviors()
    tb = typed.compile_behaviors([plain], max_emit=1, entities=entities(entity))
    assert tb.uses_sharding and len(tb.entity_types) == 2 and tb.timer_keys == 1
    rt = {"transparent": (), "starts": []}
    if sharding:
        rt["sharding"] = tb.entity_types
    return wl.Workload("sharding_kat", N_KAT, 2, 1, T, capacity, [(f, c, tb.kind_of(plain), None) for f, c in PLAIN], behaviors=tb,
                       outbound=(HOST, 1), bucket_actors=32, timers={"n_keys": tb.timer_keys, "receive_timeout": rt})


def scenario_workload(name: str, T: int) -> wl.Workload:
    sc = SCENARIOS[name]
    return kat_workload(sc.get("throughput", T), sc.get("capacity", 0))


def counts(st) -> dict:
    return {k: (st[k] if isinstance(st, dict) else getattr(st, k)) for k in COUNT_KEYS}


def conserved(st: dict, timer_info: dict, rt_info: dict) -> bool:
    """staged + emitted + timer fired + receive-timeout fired = delivered + dead_letters + in_flight (§2.7's)"""
    return st["staged"] + st["emitted"] + timer_info["fired"] + rt_info["fired"] == \
        st["delivered"] + st["dead_letters"] + st["in_flight"]


def tell_pairs(target, pairs) -> None:
    if pairs:
        dst = np.asarray([d for d, _ in pairs], np.uint32)
        pay = np.asarray([payload(m) for _, m in pairs], np.uint32)
        target.tell(dst, pay, np.full(dst.size, NO_SENDER, np.uint32))


def ordered(d, s, p):
    """the outbox as [sender, payload] pairs in canonical order: by sender, each sender's messages in its order"""
    o = per_sender(d, s, p)
    return [[int(a), int(b)] for a, b in zip(o[0].tolist(), o[2].tolist())]


def snapshot(target, st) -> dict:
    """everything observable: counters, the three infos, every id's entity row and timeout, state words, alive flags,
    the outbox"""
    st = counts(st)
    ti, ri, si = target.timer_info(), target.receive_timeout_info(), target.sharding_info()
    assert conserved(st, ti, ri), (st, ti, ri)
    r, e = target.read_receive_timeout(), target.read_entities()
    words, alive = target.read_state()
    return dict(counts=st, timer_info=ti, rt_info=ri, info=si, rt={k: r[k].tolist() for k in ("delay", "remaining", "payload")},
                entities={k: e[k].tolist() for k in ("alive", "incarnations", "passivating")},
                words=words.tolist(), alive=(alive & 1).tolist(), echo=ordered(*target.take_outbound()))


def run_kat(name: str, T: int, target) -> dict:
    """Run the scenario's script on `target` (an engine or the model, the workload applied): per step the echoes, the
    ticks and the probe, then the final counters, infos, entity rows and state words of the ids the scenario names."""
    sc = SCENARIOS[name]
    echo, ticks, probes, st = [], [], [], None
    for step in sc["script"]:
        tell_pairs(target, step["tell"])
        st = counts(target.run() if step["run"] is None else target.run(step["run"]))
        echo.append(ordered(*target.take_outbound()))
        ticks.append(target.timer_info()["ticks"])
        assert conserved(st, target.timer_info(), target.receive_timeout_info()), (name, T, st)
        pr = step.get("probe")
        if pr:
            e, r = target.read_entities(pr["id"], 1), target.read_receive_timeout(pr["id"], 1)
            got = dict(id=pr["id"], entity=[int(e[k][0]) for k in ("alive", "incarnations", "passivating")], delay=int(r["delay"][0]))
            if "remaining" in pr:
                got["remaining"] = int(r["remaining"][0])
            probes.append(got)
    words, alive = target.read_state()
    ids = sorted(int(i) for i in sc["final"]["entities"])
    ent = {}
    for i in ids:
        e = target.read_entities(i, 1)
        assert int(e["alive"][0]) == int(alive[i] & 1)
        ent[str(i)] = [int(e[k][0]) for k in ("alive", "incarnations", "passivating")]
    return dict(echo=echo, ticks=ticks, probes=probes, counts=st, sharding=target.sharding_info(),
                timer_fired=target.timer_info()["fired"], rt_fired=target.receive_timeout_info()["fired"], entities=ent,
                words={str(i): [int(words[i, 0]), int(words[i, 1])] for i in ids})


def per_T(v, T: int):
    """a value of the JSON that differs by throughput is written {"1": .., "2": .., "16": ..}"""
    return v[str(T)] if isinstance(v, dict) and set(v) == {str(t) for t in KAT_T} else v


def check_kat(name: str, T: int, got: dict) -> None:
    """`got` against the JSON."""
    sc = SCENARIOS[name]
    want_echo = [[[s, payload(m)] for s, m in e] for e in per_T(sc["echo"], T)]
    assert got["echo"] == want_echo, (got["echo"], want_echo)
    assert got["ticks"] == [per_T(t, T) for t in sc["ticks"]], (got["ticks"], sc["ticks"])
    assert got["probes"] == [s["probe"] for s in sc["script"] if "probe" in s], got["probes"]
    f = sc["final"]
    assert got["sharding"] == f["sharding"], got["sharding"]
    assert got["counts"]["dead_letters"] == per_T(f["dead_letters"], T) and got["counts"]["in_flight"] == 0, got["counts"]
    assert got["timer_fired"] == f["timer_fired"] and got["rt_fired"] == f["rt_fired"], got
    assert got["entities"] == f["entities"], got["entities"]
    assert got["words"] == f["words"], got["words"]


# ------------------------------------------------------------------ the seeded workloads, at the sizes the GPU tests use
def seeded_workloads() -> dict:
    """name -> workload: 96 to 200 entities in buckets of 32 beside 8 registered plain actors (the entity range starts
    at id 8: it crosses every bucket boundary it meets)."""
    return {
        "sharded_entities_T16": wl.sharded_entities(150, idle=3, ticks=40, seed=7, throughput=16, bucket_actors=32,
                                                    p_passivate=0.04, p_stop=0.02),
        "sharded_entities_T1": wl.sharded_entities(96, idle=3, ticks=40, seed=11, throughput=1, bucket_actors=32,
                                                   p_passivate=0.04, p_stop=0.02),
        "passivation_race_T1": wl.passivation_race(200, idle=2, throughput=1, bucket_actors=32),
        "passivation_race_T16": wl.passivation_race(200, idle=2, throughput=16, bucket_actors=32),
    }
