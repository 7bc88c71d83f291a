"""The plain model of LWWMap delta replication (tests/lwwmap_delta_model.py), without a GPU: the known answers of
tests/golden/lwwmap_delta_kats.json, the model's ORSet mergeDelta against the existing ORSetSpec fixture,
mergeDelta against the full-state merge, the canonical form, the engine's constants, and the census of what the
seeded GPU cases (tests/lwwmap_delta_cases.py) exercise."""
import json
import pathlib

import numpy as np
import pytest

from akka_amd import engine as E
from akka_amd import workloads as wl
from akka_amd.ddata import LWWMap as DecodedMap
from akka_amd.engine import Kind, Op
from tests import crdt_model as M
from tests import lwwmap_delta_cases as CS
from tests import lwwmap_delta_model as D
from tests import lwwmap_model as L

GOLD = pathlib.Path(__file__).resolve().parent / "golden"


def test_constants_and_public_surface():
    """What the feature adds to the package (all missing before it)."""
    assert E.LWWMAP_DELTA_WORDS == D.DELTA_WORDS == 356 + 12 + 64 * 16 // 2 == 880
    assert E.LWWMAP_DELTA_LOG_U32 == D.ENT_U32 and E.DELTA_MAX_SIZE == 50
    assert hasattr(E.GpuEngine, "set_lwwmap_delta")
    w = wl.crdt_lwwmap_delta(16, rounds=2)
    assert w.lwwmap_delta == 50 and w.n_words == 880 and w.max_emit >= 4 and w.lwwmap == ("default", 0)
    assert wl.crdt_lwwmap(16).lwwmap_delta == 0  # (the field's default leaves the other workloads alone)
    hdr = (GOLD.parent.parent / "include" / "akka_gpu.h").read_text()
    assert "agx_set_lwwmap_delta(agx_engine* eng, uint32_t max_delta_size)" in hdr
    assert "#define AGX_LWWMAP_DELTA_LOG_U32 16u" in hdr


@pytest.mark.parametrize("case", CS.KATS["cases"], ids=lambda c: c["name"])
def test_kats(case):
    D.check_script(case, D.run_script(case))


@pytest.mark.parametrize("case", CS.KATS["engine_scripts"], ids=lambda c: c["name"])
def test_engine_scripts_on_the_model(case):
    trace = CS.run_engine_script(case, D.LwwDeltaModel(case["replicas"], max_emit=4))
    assert len(trace) == sum(1 for s in case["script"] if "expect" not in s)


def test_orset_merge_delta_against_the_orsetspec_fixture():
    """The model's ORSet deltas on tests/golden/orset_delta_kat.json (ORSetSpec "ORSet deltas")."""
    for c in json.loads((GOLD / "orset_delta_kat.json").read_text())["cases"]:
        vals, deltas, clock = {}, {}, [0]
        for op in c["ops"]:
            k = op[0]
            if k == "empty":
                vals[op[1]] = (M.ORSet(), None)
            elif k in ("add", "remove", "clear"):
                s, d0 = vals[op[2]]
                if k == "add":
                    clock[0] += 1
                    s2, d = D.orset_add(s, op[3], op[4], clock[0])
                elif k == "remove":
                    s2, d = D.orset_remove(s, op[3], op[4])
                else:
                    s2, d = D.orset_clear(s)
                vals[op[1]] = (s2, d if d0 is None else D.set_delta_merge(d0, d))
            elif k == "reset":
                vals[op[1]] = (vals[op[2]][0], None)
            elif k == "merge":
                vals[op[1]] = (vals[op[2]][0].merge(vals[op[3]][0]), None)
            elif k == "merge_delta":
                vals[op[1]] = (D.orset_merge_delta(vals[op[2]][0], deltas[op[3]]), None)
            elif k == "delta":
                assert vals[op[2]][1] is not None, (c["name"], op)
                deltas[op[1]] = vals[op[2]][1]
            elif k == "dmerge":
                deltas[op[1]] = D.set_delta_merge(deltas[op[2]], deltas[op[3]])
            else:
                raise AssertionError(op)
        for chk in c["checks"]:
            k = chk[0]
            if k == "elements":
                assert vals[chk[1]][0].element_set() == set(chk[2]), (c["name"], chk)
            elif k == "absent":
                assert chk[2] not in vals[chk[1]][0].element_set(), (c["name"], chk)
            elif k == "equal":
                assert vals[chk[1]][0] == vals[chk[2]][0], (c["name"], chk)
            elif k == "vv_has":
                assert bool(vals[chk[1]][0].vvector.get(chk[2], 0)) == chk[3], (c["name"], chk)
            elif k in ("add_op", "last_add"):
                d = deltas[chk[1]]
                assert (k == "last_add") == isinstance(d, D.SetDeltaGroup), (c["name"], chk)
                op = d.ops[-1] if isinstance(d, D.SetDeltaGroup) else d
                assert isinstance(op, D.AddDeltaOp) and set(op.underlying.elements) == set(chk[2]), (c["name"], chk)
            elif k == "group":
                d = deltas[chk[1]]
                assert isinstance(d, D.SetDeltaGroup) and len(d.ops) == chk[2], (c["name"], chk)
                want = {"add": D.AddDeltaOp, "remove": D.RemoveDeltaOp, "full": D.FullStateDeltaOp}[chk[3]]
                assert isinstance(d.ops[-1], want), (c["name"], chk)
            else:
                raise AssertionError(chk)


def _history(rng, n_ops, removes_concurrent, base_nodes=1):
    """Two replicas (nodes 0 and 1) that start equal; node 0 then applies a seeded run of puts and removes.
    Without `removes_concurrent` node 1 stays as it was (no put of its own that a remove of node 0 could miss).
    base_nodes 1: the common start was written by node 0 alone; 2: by both nodes in turn."""
    base = L.LWWMap()
    now = 0
    for i in range(6):
        now += 1
        base, _ = D.put_delta(base, i % base_nodes, int(rng.integers(0, 6)), i, L.default_clock, now)
    a, b, deltas = base, base, []
    if removes_concurrent:
        now += 1
        b, _ = D.put_delta(b, 1, 3, 999, L.default_clock, now)
    for i in range(n_ops):
        key = int(rng.integers(0, 6))
        if rng.integers(0, 4) == 0:
            a, d = D.remove_delta(a, 0, key)
        else:
            now += 1
            a, d = D.put_delta(a, 0, key, 100 + i, L.default_clock, now)
        assert a.canonical()
        deltas.append(d)
    return a, b, deltas


@pytest.mark.parametrize("max_delta", [50, 3])
def test_merge_delta_of_unsent_deltas_equals_the_full_state_merge(max_delta):
    """A peer that merges a replica's unsent deltas -- as one group, or one by one -- ends where the full-state
    merge ends, on histories without a remove concurrent with a put of the same key; the canonical form holds
    after every op."""
    rng = np.random.default_rng(11)
    groups = 0
    for _ in range(60):
        a, b, deltas = _history(rng, int(rng.integers(1, 12)), False)
        want = b.merge(a)
        one_by_one = b
        for d in deltas:
            one_by_one = D.merge_delta(one_by_one, d)
            assert one_by_one.canonical()
        assert one_by_one == want
        g = D.collect_group(deltas, max_delta)
        if g is not D.NO_DELTA:
            groups += 1
            got = D.merge_delta(b, g)
            assert got.canonical() and got == want, (deltas, got, want)
            assert D.delta_size(g) < max_delta or len(deltas) == 1
    assert groups > 10


def test_merge_delta_keeps_another_nodes_dot_that_the_full_state_merge_sheds():
    """When the common start holds dots of node 1, a put of node 0 replaces them on node 0, and the full-state merge
    sheds them on the peer (node 0's vvector has seen them).  An AddDeltaOp carries the one-node vvector of its dot
    (DD/ORSet.scala:344), so mergeDelta keeps node 1's dot beside the new one: same entries and registers, more dots."""
    rng = np.random.default_rng(11)
    more_dots = 0
    for _ in range(60):
        a, b, deltas = _history(rng, int(rng.integers(1, 12)), False, base_nodes=2)
        want = b.merge(a)
        got = b
        for d in deltas:
            got = D.merge_delta(got, d)
        assert got.canonical() and got.values == want.values and got.keys.vvector == want.keys.vvector
        assert set(got.keys.elements) == set(want.keys.elements)
        for k, dot in want.keys.elements.items():
            assert dot.items() <= got.keys.elements[k].items()
        more_dots += got.keys != want.keys
    assert more_dots > 0


def test_concurrent_put_survives_a_remove_delta():
    """The other kind of history: node 1 put key 3 concurrently; node 0's remove of key 3 does not remove it."""
    rng = np.random.default_rng(12)
    a, b, deltas = _history(rng, 0, True)
    a, d = D.remove_delta(a, 0, 3)
    got = D.merge_delta(b, d)
    assert got.canonical() and got.entries.get(3) == 999


def test_put_delta_matches_the_full_state_put():
    m = L.LWWMap()
    for i in range(10):
        m2, d = D.put_delta(m, i % 3, i % 4, i, L.default_clock, i + 1)
        assert m2 == m.put(i % 3, i % 4, i, L.default_clock, i + 1)
        assert isinstance(d, D.PutDeltaOp) and d.value == m2.values[i % 4]
        m = m2
    m2, d = D.remove_delta(m, 0, 1)
    assert m2 == m.remove(1) and d.underlying.underlying.vvector == m.keys.vvector


def test_ddata_accepts_a_delta_width_row():
    w = wl.crdt_lwwmap_delta(16, rounds=3, ops_per_replica=2)
    m = D.LwwDeltaModel(**w.engine_kwargs())
    w.apply_to(m)
    m.run()
    words, _ = m.read_state()
    assert words.shape[1] == 880
    for a in (0, 9):
        dec = DecodedMap.from_words(words[a])
        assert dec.entries == m.maps[a].entries and dec.delta_versions == tuple(m.dv[a])
        assert DecodedMap.from_words(words[a, :356]).delta_versions is None
    assert any(any(dv) for dv in m.dv)


@pytest.mark.parametrize("name", sorted(CS.CASES))
def test_census_of_the_gpu_cases(name):
    """Each seeded GPU case really contains what it claims (coalesced puts, uncoalesced groups, placeholders,
    skipped, queued and dropped propagations), on the model run."""
    _, model, st = CS.model_run(name)
    assert st["unhandled"] == 0 and not model.range_error
    CS.assert_claims(name, model)
    for a in range(model.n):
        assert model.maps[a].canonical()


def test_ring_of_65_unsent_seqnrs_is_a_capacity_error():
    w = CS.ring_fill(65)
    m = D.LwwDeltaModel(**w.engine_kwargs())
    w.apply_to(m)
    m.run()
    assert m.capacity_error
    _, m64, _ = CS.model_run("ring_64")
    assert not m64.capacity_error


def test_every_census_kind_is_claimed_by_some_case():
    claimed = {c for _, _, cl in CS.CASES.values() for c in cl if isinstance(c, str)}
    assert {"coalesced_puts", "uncoalesced_groups", "placeholders", "skipped_props", "queued_props", "dropped_props"} <= claimed


def test_convergence_on_the_model():
    w = wl.crdt_lwwmap_delta(40, rounds=4, write=True, ops_per_replica=2, bucket_actors=32)
    m = D.LwwDeltaModel(**w.engine_kwargs())
    w.apply_to(m)
    m.run()
    ids = np.arange(40, dtype=np.uint32)
    m.tell(ids, np.full(40, Op.make(Op.DELTA_TICK, 7), np.uint32))
    m.tell(ids, np.full(40, Op.make(Op.GOSSIP, 11), np.uint32))
    m.run()
    assert m.key_converged()
    for a in range(40):
        g = a & ~7
        assert all(m.dv[a][x % 8] == m.ctr[x] for x in range(g, min(g + 8, 40)) if x != a), (a, m.dv[a])
