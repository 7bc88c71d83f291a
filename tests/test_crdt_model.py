"""The plain CRDT model (tests/crdt_model.py) against the reference's known answers and against the C
restatement (oracle/crdt_ref.h), and the crafted states (tests/crdt_cases.py): join laws on every
generated state, the dials they must cover, and the Python restatement of the gossip peers."""
import json
import pathlib
import random

import numpy as np
import pytest

from akka_amd.engine import Kind, Op
from tests import crdt_cases as C
from tests import crdt_model as M

GOLD = pathlib.Path(__file__).resolve().parent / "golden"


def load(name):
    return json.loads((GOLD / name).read_text())


def _ikeys(d):
    return {int(k): v for k, v in d.items()}


# ------------------------------------------------------------------ the reference's answers
def test_model_subtract_dots_kat():
    for c in load("orset_kat.json")["subtract_dots"]:
        assert M.subtract_dots(_ikeys(c["dot"]), _ikeys(c["vvector"])) == _ikeys(c["expected"]), c["name"]


def test_model_orset_merge_kats():
    for c in load("orset_kat.json")["merges"]:
        a = M.ORSet({k: _ikeys(v) for k, v in c["this"]["elements"].items()}, _ikeys(c["this"]["vvector"]))
        b = M.ORSet({k: _ikeys(v) for k, v in c["that"]["elements"].items()}, _ikeys(c["that"]["vvector"]))
        vv = M.vv_merge(a.vvector, b.vvector)
        for m in (a.merge(b), b.merge(a)):
            assert m.elements == {k: _ikeys(v) for k, v in c["expected_elements"].items()}, c["name"]
            assert m.vvector == vv, c["name"]


def run_script(ops, new=M.ORSet, add=lambda s, node, e: s.add(node, e), remove=lambda s, e: s.remove(e),
               merge=lambda a, b: a.merge(b), copy=lambda s: s.copy()):
    """An orset_kat.json script (make_golden.py: new / add / remove / copy / merge) over any
    implementation of the five operations; elements are numbered in order of first appearance."""
    reps, idx = {}, {}
    for op in ops:
        if op[0] == "new":
            reps[op[1]] = new()
        elif op[0] == "add":
            reps[op[1]] = add(reps[op[1]], op[2], idx.setdefault(op[3], len(idx)))
        elif op[0] == "remove":
            reps[op[1]] = remove(reps[op[1]], idx.setdefault(op[2], len(idx)))
        elif op[0] == "copy":
            reps[op[1]] = copy(reps[op[2]])
        elif op[0] == "merge":
            reps[op[1]] = merge(reps[op[2]], reps[op[3]])
        else:
            raise AssertionError(op)
    return reps, {v: k for k, v in idx.items()}


def test_model_orset_scripts():
    scripts = load("orset_kat.json")["scripts"]
    assert len(scripts) == 11  # ORSetSpec "ORSet unit test" (3) and the eight "A ORSet must" cases
    for c in scripts:
        reps, inv = run_script(c["ops"])
        for chk in c["checks"]:
            assert {inv[e] for e in reps[chk[1]].element_set()} == set(chk[2]), (c["name"], chk)


def _gc(ops):
    inc, dec = {}, {}
    for op, slot, n in ops:
        if op == "inc":
            inc = M.gcounter_increment(inc, slot, n)
        else:
            dec = M.gcounter_increment(dec, slot, n)
    return inc, dec


def test_model_gcounter_kats():
    g = load("gcounter_kat.json")
    slots = g["slots"]
    for case in g["cases"]:
        c = _gc(case["ops"])[0]
        assert M.gcounter_to_words(c, slots).tolist() == case["state"], case["name"]
        if "value" in case:
            assert M.gcounter_value(c) == case["value"]
    for m in g["merges"]:
        a, b = _gc(m["a_ops"])[0], _gc(m["b_ops"])[0]
        assert M.gcounter_to_words(a, slots).tolist() == m["a_state"] and M.gcounter_value(a) == m["a_value"]
        assert M.gcounter_to_words(b, slots).tolist() == m["b_state"] and M.gcounter_value(b) == m["b_value"]
        for x, y in ((a, b), (b, a)):
            mg = M.gcounter_merge(x, y)
            assert M.gcounter_to_words(mg, slots).tolist() == m["merged_state"], m["name"]
            assert M.gcounter_value(mg) == m["merged_value"], m["name"]


def test_model_pncounter_kats():
    g = load("pncounter_kat.json")
    slots = g["slots"]
    for case in g["cases"]:
        c = _gc(case["ops"])
        if "increments" in case:
            assert M.gcounter_to_words(c[0], slots).tolist() == case["increments"], case["name"]
            assert M.gcounter_to_words(c[1], slots).tolist() == case["decrements"], case["name"]
        if "value" in case:
            assert M.gcounter_value(c[0]) == case["increments_value"], case["name"]
            assert M.gcounter_value(c[1]) == case["decrements_value"], case["name"]
            assert M.pncounter_value(c) == case["value"], case["name"]
    for m in g["merges"]:
        a, b = _gc(m["a_ops"]), _gc(m["b_ops"])
        assert M.pncounter_value(a) == m["a_value"] and M.pncounter_value(b) == m["b_value"]
        for x, y in ((a, b), (b, a)):
            mg = M.pncounter_merge(x, y)
            assert M.gcounter_value(mg[0]) == m["merged_increments_value"], m["name"]
            assert M.gcounter_value(mg[1]) == m["merged_decrements_value"], m["name"]
            assert M.pncounter_value(mg) == m["merged_value"], m["name"]


def test_model_versionvector_kats():
    """Every case of versionvector_kat.json (the merge cases and the comparisons they rest on)."""
    n_merge = 0
    for c in load("versionvector_kat.json")["cases"]:
        vs, clock = {}, 0
        for op in c["ops"]:
            if op[0] == "new":
                vs[op[1]] = {}
            elif op[0] == "copy":
                vs[op[1]] = dict(vs[op[2]])
            elif op[0] == "inc":  # one global counter, as Timestamp.counter
                clock += 1
                vs[op[1]] = {**vs[op[2]], op[3]: clock}
            elif op[0] == "merge":
                vs[op[1]] = M.vv_merge(vs[op[2]], vs[op[3]])
                n_merge += 1
        for chk in c["checks"]:
            k = chk[0]
            if k == "size":
                assert len(vs[chk[1]]) == chk[2], (c["name"], chk)
            elif k == "contains":
                assert (chk[2] in vs[chk[1]]) == chk[3], (c["name"], chk)
            elif k == "cmp":
                assert (M.vv_compare(vs[chk[1]], vs[chk[2]]) == chk[3]) == chk[4], (c["name"], chk)
            elif k == "gt_at":
                assert M.vv_version_at(vs[chk[1]], chk[3]) > M.vv_version_at(vs[chk[2]], chk[3]), (c["name"], chk)
            elif k == "eq_at":
                assert M.vv_version_at(vs[chk[1]], chk[3]) == M.vv_version_at(vs[chk[2]], chk[3]), (c["name"], chk)
    assert n_merge >= 5


def test_words_round_trip():
    for s in C.pool().values():
        assert M.orset_from_words(M.orset_to_words(s)) == s
    g = {0: 2**64 - 1, 3: 2**32, 7: 1}
    assert M.gcounter_from_words(M.gcounter_to_words(g)) == g
    p = (g, {1: 2**32 - 1})
    assert M.pncounter_from_words(M.pncounter_to_words(p)) == p
    with pytest.raises(AssertionError):  # the model does not wrap: a version past the field is refused
        M.orset_to_words(M.ORSet({0: {0: 2**32}}, {0: 2**32}))


# ------------------------------------------------------------------ crafted states
def test_crafted_dials():
    """Every dial of tests/crdt_cases.py is covered by a generated replica."""
    p = C.pool()
    live = {k: sum(len(d) for d in s.elements.values()) for k, s in p.items()}
    assert live["empty"] == 0 and not p["empty"].vvector
    assert live["single_dot"] == 1
    assert live["full511"] == 511 and live["full512"] == 512
    assert set(p["high16"].elements) == set(range(48, 64))
    assert set(p["only63"].elements) == {63} and len(p["only63"].elements[63]) == 8
    assert not p["cleared"].elements and len(p["cleared"].vvector) == 8
    states = list(p.values())
    C.assert_census(states)
    used = C.versions_used(states)
    assert all(v in used for v in C.SPECIAL_VERSIONS), [v for v in C.SPECIAL_VERSIONS if v not in used]
    assert any(v <= 15 for v in used)
    pairs = [(a, b) for a in range(len(states)) for b in range(len(states)) if a != b]
    pc = C.pair_census(states, pairs)
    assert all(pc[k] > 0 for k in ("==", "<", ">", "<>", "vanish", "stay")), pc
    assert C.pair_census(C.population(64), [(40, 41)])  # (a population is the pool, then repeats)
    assert len(C.population(64)) == 64 and C.population(64)[:len(states)] == states


def test_rescaling_keeps_every_order_relation():
    """The version map is strictly monotone per node: every comparison a merge makes (dot against
    vvector entry, dot against dot, vvector against vvector) is the same before and after."""
    raw = [s for _, s in C._history(0x5EED)]
    ij = [(i, j) for i in range(0, len(raw), 3) for j in range(1, len(raw), 4)]
    merged = [raw[i].merge(raw[j]) for i, j in ij]
    for scales in C.VARIANTS.values():
        scaled = C.rescale(raw + merged, scales)  # (a merge raises no node's last version: one map for all)
        for k, (i, j) in enumerate(ij):
            assert M.vv_compare(raw[i].vvector, raw[j].vvector) == M.vv_compare(scaled[i].vvector, scaled[j].vvector)
            assert scaled[i].merge(scaled[j]) == scaled[len(raw) + k], (i, j)  # merge commutes with the map


@pytest.mark.parametrize("variant", sorted(C.VARIANTS))
def test_model_merge_equals_c_restatement(variant):
    """On the crafted states model.merge equals oracle.orset.merge bit for bit, both ways round."""
    from oracle.oracle import orset
    states = list(C.pool(variant=variant).values())
    words = [M.orset_to_words(s) for s in states]
    for i, a in enumerate(states):
        for j, b in enumerate(states):
            assert np.array_equal(M.orset_to_words(a.merge(b)), orset.merge(words[i], words[j])), (i, j)


@pytest.mark.parametrize("variant", sorted(C.VARIANTS))
def test_join_laws_on_generated_states(variant):
    """Merging a list of generated states gives the same result in the given order, the reverse and 20
    seeded shuffles, and merging is idempotent -- for every generated state and every list: the whole
    pool, a 256-replica population and 40 seeded sublists.  This is what lets a GPU test compute an
    expected state without knowing the arrival order."""
    states = list(C.pool(variant=variant).values())
    rng = random.Random(11)
    lists = [states, C.population(256, variant=variant)] + [rng.sample(states, rng.randrange(2, 7)) for _ in range(40)]
    covered = set()
    for lst in lists:
        ref = M.merge_all(lst)
        assert M.merge_all(lst[::-1]) == ref
        for k in range(20):
            sh = list(lst)
            random.Random(1000 + k).shuffle(sh)
            assert M.merge_all(sh) == ref, k
        assert ref.merge(ref) == ref
        for s in lst:
            assert s.merge(s) == s and ref.merge(s) == ref and s.merge(ref) == ref
            covered.add(id(s))
    assert all(id(s) in covered for s in states)  # 100 % of the generated states


def test_peers_match_the_oracle():
    from oracle.oracle import crdt_key_peer, crdt_peer
    rng = random.Random(5)
    for _ in range(400):
        n = rng.choice([2, 3, 8, 9, 64, 72, 256, 100_000])
        s, rnd, j, seed = rng.randrange(n), rng.randrange(0, 40), rng.randrange(4), rng.getrandbits(64)
        assert C.crdt_peer(seed, s, rnd, j, n) == crdt_peer(seed, s, rnd, j, n), (seed, s, rnd, j, n)
        if min(8, n - (s & ~7)) > 1:
            assert C.crdt_key_peer(seed, s, rnd, j, n) == crdt_key_peer(seed, s, rnd, j, n), (seed, s, rnd, j, n)
    assert C.crdt_peer(C.seed_for(0, 1, 3), 0, 0, 0, 3) == 1


def test_counter_population_covers_both_halves():
    for kind in (Kind.GCOUNTER, Kind.PNCOUNTER):
        w = C.counter_population(kind, 64)
        pairs = [(s, r) for r, ss in C.senders(64, 7, 2, 0, False).items() for s in ss]
        C.assert_counter_census(w, pairs)
        if kind == Kind.PNCOUNTER:  # both halves independently
            C.assert_counter_census(w[:, :8], pairs)
            C.assert_counter_census(w[:, 8:], pairs)


# ------------------------------------------------------------------ the oracle refuses a version wrap
def test_oracle_refuses_orset_version_wrap():
    """The reference's versions are Long and never wrap; the u32 entry of the engine layout would.
    oracle.orset.add and the BSP oracle refuse the add at 2^32 - 1 (the engine: AGX_ERANGE)."""
    from oracle import BspOracle
    from oracle.oracle import orset
    w = M.orset_to_words(M.ORSet({5: {3: 2**32 - 2}}, {3: 2**32 - 2}))
    w = orset.add(w, 3, 5)
    assert M.orset_from_words(w) == M.ORSet({5: {3: 2**32 - 1}}, {3: 2**32 - 1})
    with pytest.raises(OverflowError):
        orset.add(w, 3, 5)
    for delta in (False, True):
        wk = C.workload([(Kind.ORSET, np.stack([w] * 8))], ([3], [Op.make(Op.ADD, 9)]), delta=delta, fanout=1)
        o = BspOracle(**wk.engine_kwargs())
        wk.apply_to(o)
        with pytest.raises(OverflowError, match="2\\^32"):
            o.run()
        ws, _ = o.read_state()
        assert M.orset_from_words(ws[3]).vvector == {3: 2**32 - 1}  # the version vector did not go backwards
        o.close()
        wk = C.workload([(Kind.ORSET, np.stack([w] * 8))], ([2], [Op.make(Op.ADD, 9)]), delta=delta, fanout=1)
        o = BspOracle(**wk.engine_kwargs())
        wk.apply_to(o)
        o.run()  # node 2's entry is 0: an ordinary add
        assert M.orset_from_words(o.read_state()[0][2]).elements[9] == {2: 1}
        o.close()
