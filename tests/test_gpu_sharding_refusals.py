"""The refusals of sharded entities (agx_set_sharding), each with its status and text; afterwards the
engine still runs and equals an engine that never saw the refused call."""
import numpy as np
import pytest

from akka_amd import typed
from akka_amd._lib import AgxError
from akka_amd.engine import EngineConfig, GpuEngine, Kind
from tests import sharding_cases as sc

pytestmark = pytest.mark.gpu

EINVAL, ESTATE = 1, 6
SCRIPT = [[(37, "Job"), (55, "Job"), (3, "Fwd:41")], [(37, "Passivate"), (41, "Job")], [(37, "Job"), (37, "Job")], []]


def status_and_text(call):
    with pytest.raises(AgxError) as e:
        call()
    return e.value.status, str(e.value).split(": ", 1)[1]   # ("AGX_EINVAL: <the engine's text>")


def bare(w, upto="receive_timeout"):
    """an engine with the workload's actors and tables and the features up to `upto`, sharding not set"""
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    for first, count, kind, init in w.ranges:
        eng.register_range(first, count, kind, init)
    eng.set_outbound(*w.outbound)
    eng.set_behaviors(w.behaviors)
    if upto in ("timers", "receive_timeout"):
        eng.set_timers(w.timers["n_keys"])
    if upto == "receive_timeout":
        eng.set_receive_timeout(())
    return eng


def run_script(eng):
    out = []
    for step in SCRIPT:
        sc.tell_pairs(eng, step)
        out.append(sc.snapshot(eng, eng.run(2)))
    eng.close()
    return out


@pytest.fixture(scope="module")
def untouched(built):
    """the script on an engine that never saw a refused call"""
    w = sc.kat_workload(2)
    eng = bare(w)
    eng.set_sharding(w.behaviors.entity_types)
    out = run_script(eng)
    assert out[-1]["info"]["restarted"] == 1 and out[-1]["info"]["started"] == 4
    return out


def types_of(w):
    return [list(t) for t in w.behaviors.entity_types]


def test_call_order(built, untouched):
    w = sc.kat_workload(2)
    text = "sharding needs an engine with receive timeouts (agx_set_timers, then agx_set_receive_timeout first)"
    eng = bare(w, upto="none")
    assert status_and_text(lambda: eng.set_sharding(w.behaviors.entity_types)) == (EINVAL, text)
    eng.set_timers(1)
    assert status_and_text(lambda: eng.set_sharding(w.behaviors.entity_types)) == (EINVAL, text)
    eng.set_receive_timeout(())
    eng.set_sharding(w.behaviors.entity_types)
    assert status_and_text(lambda: eng.set_ask())[0] == EINVAL   # (the ask pattern and receive timeouts exclude one another)
    assert run_script(eng) == untouched


def test_second_call(built, untouched):
    w = sc.kat_workload(2)
    eng = bare(w)
    eng.set_sharding(w.behaviors.entity_types)
    assert status_and_text(lambda: eng.set_sharding(w.behaviors.entity_types)) == \
        (EINVAL, "sharding is set already (agx_set_sharding is called once)")
    assert run_script(eng) == untouched


def test_after_the_first_run(built):
    cfg = dict(n_actors=64, throughput=3, capacity=0, n_words=2, max_emit=1, bucket_actors=32)
    types = [(40, 8, typed.KIND_COMPILED, 0, None, sc.payload("Bye"), 0, 0)]
    out = []
    for refused in (True, False):
        eng = GpuEngine(EngineConfig(**cfg))
        eng.register_range(0, 40, Kind.COUNTER)
        eng.set_timers(1)
        eng.set_receive_timeout(())
        eng.tell(1, 1)
        eng.run()
        if refused:
            assert status_and_text(lambda: eng.set_sharding(types)) == (ESTATE, "set sharding before the first agx_run")
        eng.tell(np.asarray([42, 2], np.uint32), 1)   # (no sharding on either: a tell to an unregistered id is a dead letter)
        st = eng.run()
        out.append((sc.counts(st), eng.read_state()[0].tolist(), eng.sharding_info(), eng.read_entities(40, 8)["incarnations"].tolist()))
        eng.close()
    assert out[0] == out[1] and out[0][0]["dead_letters"] == 1 and out[0][2] == dict.fromkeys(sc.SHARD_KEYS, 0)


@pytest.mark.parametrize("case", ["overlap", "out_of_range", "empty", "none", "too_many"])
def test_bad_ranges(built, untouched, case):
    w = sc.kat_workload(2)
    t = types_of(w)
    eng = bare(w)
    if case == "overlap":
        t[1][0], t[1][1] = 40, 10
        want = "sharding: the ranges of entity types 0 and 1 overlap"
    elif case == "out_of_range":
        t[1][0], t[1][1] = 60, 21
        want = "sharding: entity type 1 is empty or leaves [0, n_actors)"
    elif case == "empty":
        t[0][1] = 0
        want = "sharding: entity type 0 is empty or leaves [0, n_actors)"
    elif case == "none":
        t = []
        want = "sharding: 0 entity types (1..8)"
    else:
        t = [[44 + i % 6, 1] + t[0][2:] for i in range(9)]
        want = "sharding: 9 entity types (1..8)"
    assert status_and_text(lambda: eng.set_sharding(t)) == (EINVAL, want)
    eng.set_sharding(w.behaviors.entity_types)
    assert run_script(eng) == untouched


def test_registered_id_in_a_range_either_order(built, untouched):
    w = sc.kat_workload(2)
    plain = w.ranges[0][2]
    eng = bare(w)
    eng.register_range(43, 2, plain)   # (id 43 is the counter type's last)
    assert status_and_text(lambda: eng.set_sharding(w.behaviors.entity_types)) == \
        (EINVAL, "sharding: id 43 of entity type 0's range is registered")
    eng.close()
    eng = bare(w)
    eng.set_sharding(w.behaviors.entity_types)
    assert status_and_text(lambda: eng.register_range(43, 2, plain)) == \
        (EINVAL, "register_range [43, 45) overlaps the entity range [20, 44) (agx_set_sharding): its entities are started by "
         "their first message")
    assert status_and_text(lambda: eng.register_range(69, 1, plain))[0] == EINVAL
    eng.register_range(44, 6, plain)   # (between the ranges: free ids)
    eng.register_range(44, 6, 0)       # (and gone again: Kind.NONE)
    assert run_script(eng) == untouched


def test_non_compiled_kind_and_flags(built, untouched):
    w = sc.kat_workload(2)
    eng = bare(w)
    t = types_of(w)
    t[0][2] = 1   # (a built-in kind)
    assert status_and_text(lambda: eng.set_sharding(t)) == \
        (EINVAL, "sharding: entity type 0: kind 1 is no compiled behaviour kind, or unknown flags")
    t = types_of(w)
    t[1][5] = 0xFB000000   # (a stop message with the receive-timeout envelope's tag)
    assert status_and_text(lambda: eng.set_sharding(t)) == \
        (EINVAL, "sharding: entity type 1: a stop or idle message carries a reserved tag (0xFF, 0xFB)")
    t = types_of(w)
    t[1][2] = typed.KIND_COMPILED + 40   # (a compiled kind the tables do not hold: agx_run's refusal)
    eng.set_sharding(t)
    sc.tell_pairs(eng, [(1, "Job")])
    assert status_and_text(lambda: eng.run()) == \
        (EINVAL, "sharding: an entity type's kind 56 is no compiled behaviour of the tables (2 behaviours)")
    eng.close()
    eng = bare(w)
    eng.set_sharding(w.behaviors.entity_types)
    assert run_script(eng) == untouched


def test_passivate_without_the_feature(built):
    """tables with AGX_A_PASSIVATE on an engine with receive timeouts and no sharding: agx_run returns AGX_EINVAL"""
    w = sc.kat_workload(2)
    eng = bare(w)
    sc.tell_pairs(eng, [(1, "Job")])
    assert status_and_text(lambda: eng.run()) == \
        (EINVAL, "the compiled behaviours passivate, but the engine has no sharding (agx_set_sharding)")
    eng.set_sharding(w.behaviors.entity_types)   # (before the first run still: the refused run did not start the engine)
    st = eng.run()
    eng.close()
    assert st.delivered == 1 and st.dead_letters == 0


def test_passivate_beside_a_tell(built, untouched):
    """the DSL refuses it (tests/test_typed_sharding.py); tables written by hand are refused by agx_set_behaviors"""
    w = sc.kat_workload(2)
    tb = w.behaviors
    c = next(c for c in range(int(tb.first[-1])) if tb.cases[c].act_count == 2 and
             tb.acts[tb.cases[c].act_first + 1].op == typed.A_TELL and tb.acts[tb.cases[c].act_first].op == typed.A_ADD)
    tb.acts[tb.cases[c].act_first].op = typed.A_PASSIVATE
    eng = GpuEngine(EngineConfig(**w.gpu_kwargs()))
    assert status_and_text(lambda: eng.set_behaviors(tb)) == \
        (EINVAL, f"compiled behaviours: case {c} holds 2 of tell and passivate; an engine with sharding has max_emit 1")
    eng.close()
    w = sc.kat_workload(2)
    eng = bare(w)
    eng.set_sharding(w.behaviors.entity_types)
    assert run_script(eng) == untouched
