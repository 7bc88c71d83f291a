"""The model of sharded entities (tests/sharding_model.py) against the known answers worked out by
hand from akka-cluster-sharding's Shard.scala (tests/golden/sharding_kats.json; no JVM is available to record them),
against the receive timeouts' model where no entity type is declared, and the guards that the seeded workloads of the
GPU tests reach the paths they are there for.  No GPU."""
import numpy as np
import pytest

from akka_amd import workloads as wl
from tests import sharding_cases as sc
from tests.receive_timeout_model import ReceiveTimeoutModel
from tests.sharding_model import ShardingModel

BUCKET = 32


def model_for(w):
    m = ShardingModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


@pytest.mark.parametrize("T", sc.KAT_T)
@pytest.mark.parametrize("name", sc.KAT_NAMES)
def test_known_answers(name, T):
    got = sc.run_kat(name, T, model_for(sc.scenario_workload(name, T)))
    print(got)
    sc.check_kat(name, T, got)


def test_every_answer_has_its_citation():
    assert len(sc.KAT_NAMES) == 9
    for s in sc.SCENARIOS.values():
        assert "scala:" in s["cite"], s["name"]


def test_without_entity_types_it_is_the_receive_timeout_model():
    w = wl.passivating_entities(96, 3, idle=3)
    a, b = model_for(w), ReceiveTimeoutModel(**w.engine_kwargs())
    w.apply_to(b)
    for dst, src, pay in w.schedule:
        for m in (a, b):
            if len(dst):
                m.tell(dst, pay, src)
        sa, sb = a.run(1), b.run(1)
        assert sa == sb and a.receive_timeout_info() == b.receive_timeout_info() and a.timer_info() == b.timer_info()
        assert all(np.array_equal(x, y) for x, y in zip(a.read_state(), b.read_state()))
    assert a.run() == b.run() and a.timer_info() == b.timer_info()
    assert all(np.array_equal(x, y) for x, y in zip(a.read_state(), b.read_state()))
    assert a.sharding_info() == dict.fromkeys(sc.SHARD_KEYS, 0) and not a.read_entities()["incarnations"].any()


class Watched(ShardingModel):
    """the model, noting which paths a run takes"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.seen = dict(buffered_restart=0, plain_stop_dead=0, idle_entity_bucket=0)

    def step(self):
        before = dict(self.sh), self.c["dead_letters"], [a for a, *_ in self.backlog]
        held = {a: h for a, h in enumerate(self.held) if h} if self.held else {}
        if not super().step():
            return False
        # a restart whose mail was queued behind the stop: the entity had backlog when it started again
        if self.sh["restarted"] > before[0]["restarted"]:
            self.seen["buffered_restart"] += any(self.pst[a] == self.now - 1 and self.alive[a] for a in before[2])
        # a dead letter of a plain stop: mail an entity's plain stop left queued died at this formation
        self.seen["plain_stop_dead"] += sum(held.values()) > 0
        sizes = self.inbox_sizes[-1]
        for b in range((self.n + BUCKET - 1) // BUCKET):
            lo, hi = b * BUCKET, min((b + 1) * BUCKET, self.n)
            has_entity = any(self._type_of(a) is not None for a in range(lo, hi))
            self.seen["idle_entity_bucket"] += has_entity and sizes.sum() > 0 and sizes[lo:hi].sum() == 0
        return True


def test_seeded_workloads_reach_their_paths():
    """over the seeded workloads at the sizes the GPU tests use: an entity with at least 3 incarnations, a restart with
    buffered mail, an ignored Passivate, a dead letter from a plain stop, an entity range that crosses a bucket
    boundary, a bucket with entities and no mail"""
    seen, info, inc = dict(buffered_restart=0, plain_stop_dead=0, idle_entity_bucket=0), dict.fromkeys(sc.SHARD_KEYS, 0), 0
    for name, w in sc.seeded_workloads().items():
        assert w.bucket_actors == BUCKET and 96 <= w.behaviors.entity_types[0][1] <= 200
        first, count = w.behaviors.entity_types[0][:2]
        assert first % BUCKET and first // BUCKET != (first + count - 1) // BUCKET, "the range crosses a bucket boundary"
        m = Watched(**w.engine_kwargs())
        w.apply_to(m)
        st = w.run_schedule(m)
        assert st["in_flight"] == 0 and sc.conserved(st, m.timer_info(), m.receive_timeout_info())
        i = m.sharding_info()
        assert i["alive"] == 0 and i["passivated"] <= i["passivations"] and i["restarted"] <= i["started"], (name, i)
        print(name, i, m.seen, max(m.inc))
        for k in seen:
            seen[k] += m.seen[k]
        for k in info:
            info[k] += i[k]
        inc = max(inc, max(m.inc))
    assert inc >= 3 and seen["buffered_restart"] and info["passivate_ignored"] and seen["plain_stop_dead"]
    assert seen["idle_entity_bucket"] and info["restarted"] and info["passivate_unknown"] == 0


def test_each_race_workload_restarts_at_both_throughputs():
    for name in ("passivation_race_T1", "passivation_race_T16"):
        w = sc.seeded_workloads()[name]
        m = Watched(**w.engine_kwargs())
        w.apply_to(m)
        w.run_schedule(m)
        assert m.seen["buffered_restart"] and m.sharding_info()["restarted"] >= 100, name


def test_a_plain_actor_that_passivates_is_unknown():
    m = model_for(sc.kat_workload(3))
    sc.tell_pairs(m, [(5, "Passivate"), (37, "Job")])
    st = m.run()
    assert m.sharding_info() == dict(started=1, restarted=0, passivations=0, passivated=0, passivate_ignored=0,
                                     passivate_unknown=1, alive=1)
    assert st["emitted"] == 0 and st["dead_letters"] == 0


def test_a_forwarded_job_starts_an_entity_and_its_own_tell_does_not():
    """a plain actor's tell is a starting item; SelfTell's Job reaches the live entity; after a plain stop the entity's
    own Job is a dead letter and the forwarded one starts a new incarnation"""
    m = model_for(sc.kat_workload(16))
    sc.tell_pairs(m, [(3, "Fwd:41")])
    m.run()
    assert m.read_entities(41, 1)["incarnations"][0] == 1 and int(m.words[41, 0]) == 1
    sc.tell_pairs(m, [(41, "SelfStop"), (3, "Fwd:41")])
    st = m.run()   # tick 3: SelfStop and the forward; tick 4: the entity's own Job dies, the forwarded Job starts it
    assert st["dead_letters"] == 1 and m.read_entities(41, 1)["incarnations"][0] == 2 and int(m.words[41, 0]) == 1
    assert m.sharding_info()["restarted"] == 0
