"""The conformance program of the compiled-behaviour rule on the GPU (DESIGN.md §8 "The compiled rule at 64-bit
edges"; tests/compiled_core_cases.py has the program, tests/compiled_core_model.py the rule).  Every comparison is
bit-exact: state words, alive flags, kinds, every counter and conservation -- against the core model's fold, against
BspOracle and PrioModel (the plain engine) or against the feature's own model (the feature engines).

Which copy of the rule in akka_amd/csrc/agx_device.h a test reaches (a feature variant first shows that its engine
is that variant by a call that only such an engine answers so, compiled_core_cases.Variant.witness -- mostly the refusal
of another feature, whose text names the one that is on; test_witness_tells_the_variant_from_a_plain_engine shows that
an engine without the feature answers otherwise):
  test_plain, test_tiny_wave, test_bounded_tail_drop, test_loopback_ranks   compiled_apply
  test_feature_variant[stash]                                               compiled_apply<kStash>
  test_feature_variant[priority]                                            compiled_apply (the prioritised launch)
  test_feature_variant[timers | receive_timeout | ask | sharding]           compiled_apply_tm, <kIdle>, <kAsk>, <kIdle, kShard>
  test_feature_variant[watch]                                               compiled_apply_w
  test_feature_variant[children]                                            compiled_apply_c
  test_feature_variant[supervision | backoff]                               compiled_apply_s
  test_feature_variant[receptionist]                                        compiled_apply_rc
  test_feature_variant[topics]                                              compiled_apply_tp
  test_feature_variant[listings]                                            compiled_apply_ls
  test_feature_variant[router_logics]                                       compiled_apply_hr"""
import functools

import numpy as np
import pytest

from akka_amd._lib import AgxError
from akka_amd.engine import EngineConfig, GpuEngine, owner
from tests import compiled_core_cases as C
from tests.test_compiled_core_model import assert_core, references
from tests.test_gpu_between_runs import PIPELINES, setenv
from tests.test_gpu_parity import COUNT_KEYS

pytestmark = pytest.mark.gpu
QUIET = 1 << 30
LEGS = (2, QUIET)  # a boundary with mail in flight, then to quiescence
SHARDED_KEYS = tuple(k for k in COUNT_KEYS if k != "supersteps")


def config(w, **cfg):
    return EngineConfig(**dict(w.gpu_kwargs(), **cfg))


def legs_of(target, w, run=None):
    """per leg: (counters, words, alive, kinds)"""
    out = []
    for b in LEGS:
        st = run(b) if run else target.run(b)
        st = st if isinstance(st, dict) else {k: getattr(st, k) for k in COUNT_KEYS}
        out.append((st,) + tuple(target.read_state()) + (target.read_kinds(),))
    return out


@functools.lru_cache(maxsize=None)
def oracle_legs(throughput, n_words, bounded=False):
    from oracle import BspOracle
    prog = C.program()
    w = C.workload(prog, throughput, n_words, bounded=bounded)
    ref = BspOracle(**w.engine_kwargs())
    w.apply_to(ref)
    legs = legs_of(ref, w)
    ref.close()
    assert legs[0][0]["in_flight"] > 0 and legs[1][0]["in_flight"] == 0
    if bounded:  # (both chains are back at the behaviour they started in when their four places are used up)
        assert legs[0][0]["dead_letters"] >= 13, "the chains' mailboxes dropped nothing"
    else:
        assert (legs[0][3] != np.asarray(prog.kind, np.uint8)).any(), "no become stands at the boundary"
    return legs


def conserved(st):
    return st["staged"] + st["emitted"] == st["delivered"] + st["dead_letters"] + st["in_flight"]


def check_plain(throughput, n_words, bucket_actors, bounded=False, name=""):
    prog = C.program()
    w = C.workload(prog, throughput, n_words, bucket_actors, bounded=bounded)
    want = oracle_legs(throughput, n_words, bounded)
    eng = GpuEngine(config(w))
    try:
        w.apply_to(eng)
        got = legs_of(eng, w)
    finally:
        eng.close()
    for i, (g, r) in enumerate(zip(got, want)):
        for k in COUNT_KEYS:
            assert g[0][k] == r[0][k], f"{name} leg {i}: {k} gpu={g[0][k]} oracle={r[0][k]}"
        assert conserved(g[0]), (name, i, g[0])
        assert np.array_equal(g[2], r[2]), f"{name} leg {i}: alive differs at {np.nonzero(g[2] != r[2])[0][:8]}"
        diff = np.nonzero((g[1] != r[1]).any(axis=1))[0]
        assert diff.size == 0, (f"{name} leg {i}: state differs at {diff[:8]} ({[C.case_of(int(a)) for a in diff[:4]]}) "
                                f"gpu={[[hex(int(x)) for x in row] for row in g[1][diff[:3]]]} "
                                f"oracle={[[hex(int(x)) for x in row] for row in r[1][diff[:3]]]}")
        assert np.array_equal(g[3], r[3]), f"{name} leg {i}: kinds differ at {np.nonzero(g[3] != r[3])[0][:8]}"
    st, words, alive, kinds = got[-1]
    # the core model's fold, and the Python BSP model (two words: a third stays as registered)
    _, _, (sm, wm, am, km), cr = references(False, throughput, bounded)
    assert_core(cr, st, words, alive, kinds, f"{name} core")
    for k in COUNT_KEYS:
        assert st[k] == sm[k], (name, k, st[k], sm[k])
    assert np.array_equal(words[:, :2], wm) and np.array_equal(alive, am) and np.array_equal(kinds, km)
    for x in range(2, n_words):
        for a in range(C.N):
            assert int(words[a, x]) == (C.third_word(a, x) if prog.kind[a] else 0), (name, a, x, hex(int(words[a, x])))


@pytest.mark.parametrize("n_words", [2, 3])
@pytest.mark.parametrize("bucket_actors", [32, 0])
@pytest.mark.parametrize("throughput", [1, 3])
@pytest.mark.parametrize("pipe", list(PIPELINES))
def test_plain(built, monkeypatch, pipe, throughput, bucket_actors, n_words):
    """the whole program (two tells in one case included) on the plain engine: compiled_apply"""
    setenv(monkeypatch, PIPELINES[pipe])
    check_plain(throughput, n_words, bucket_actors, name=f"{pipe} T={throughput} ba={bucket_actors} W={n_words}")


@pytest.mark.parametrize("launch", ["1", "0"])
@pytest.mark.parametrize("tiny", [0, 128])
def test_tiny_wave(built, monkeypatch, launch, tiny):
    """the settings of test_tiny_wave_path_compiled: the wave launch and the block launch of the multi-pass pipeline"""
    setenv(monkeypatch, {"AGX_RADIX_BITS": "3", "AGX_TINY": str(tiny), "AGX_TINY_LAUNCH": launch, "AGX_RING_APPLY": "0"})
    check_plain(3, 2, 64, name=f"tiny={tiny} launch={launch}")


@pytest.mark.parametrize("pipe", ["fused", "bits3_ring1", "unfused"])
def test_bounded_tail_drop(built, monkeypatch, pipe):
    """the become chains behind a mailbox of four places: eleven and ten tells are staged, the chain runs A -> B -> C -> A on the
    first three, the fourth meets A again, the rest are dead letters"""
    setenv(monkeypatch, PIPELINES[pipe])
    check_plain(3, 2, 32, bounded=True, name=f"bounded {pipe}")


RANKS = 3


def test_loopback_ranks(built):
    """three loopback ranks: (self + dk) mod n wraps by the global population (the probes 0, 216 and n - 1 lie on
    different ranks than the sinks they reach), every probe's recorder is 216 ids on"""
    from oracle import BspOracle
    prog = C.program()
    w = C.workload(prog, 3)
    ref = BspOracle(n_ranks=RANKS, **w.engine_kwargs())
    w.apply_to(ref)
    so = ref.run()
    wo, ao = ref.read_state()
    ref.close()
    own_of = np.array([owner(i, 1000, RANKS) for i in range(C.N)])
    assert len({int(own_of[s]) for s in C.S_IDS} | {int(own_of[1]), int(own_of[C.N - 2])}) > 1
    engs = [GpuEngine(config(w, n_ranks=RANKS, rank=r)) for r in range(RANKS)]
    try:
        for e in engs:
            w.apply_to(e)
        sg = GpuEngine.group_run(engs)
        words, alive = np.zeros_like(wo), np.zeros_like(ao)
        for e in engs:
            a, b = e.read_state()
            own = own_of == e.cfg.rank
            words[own], alive[own] = a[own], b[own]
    finally:
        for e in engs:
            e.close()
    for k in SHARDED_KEYS:
        assert getattr(sg, k) == so[k], (k, getattr(sg, k), so[k])
    assert np.array_equal(alive, ao), np.nonzero(alive != ao)[0][:8]
    diff = np.nonzero((words != wo).any(axis=1))[0]
    assert diff.size == 0, (diff[:8], words[diff[:3]], wo[diff[:3]])
    cr = C.run_core(prog)
    for k in C.COUNTERS:
        assert getattr(sg, k) == cr["counts"][k], (k, getattr(sg, k), cr["counts"][k])
    for a in range(C.N):  # (agx_read_kinds is a single-rank call: the kinds show in what the later messages did)
        assert (int(words[a, 0]), int(words[a, 1]), int(alive[a]) & 1) == (*cr["words"][a], cr["alive"][a]), a


@pytest.fixture(params=["fused", "multipass"])
def pipeline(request, monkeypatch):
    if request.param == "multipass":  # (as the feature modules' fixtures)
        monkeypatch.setenv("AGX_RADIX_BITS", "3")
        monkeypatch.setenv("AGX_NO_FUSED", "1")
    return request.param


@functools.lru_cache(maxsize=None)
def variant_reference(variant):
    """the feature's model on the single-tell part, once: (variant, program, workload, counters, snapshot, the core fold)"""
    prog = C.program(True)
    v = C.variants(prog)[variant]
    prog = prog.with_host_tags_up_to(v.host_tag_limit)
    w = C.workload(prog, 3, bucket_actors=32, **v.features)
    m = C.model_of(v.model)(**w.engine_kwargs())
    w.apply_to(m)
    st = dict(m.run())
    return v, prog, w, st, C.variant_snapshot(m, v.infos), C.run_core(prog, own_tags=v.own_tags)


def test_single_tell_part_is_the_whole_but_two_tells():
    """the census of tests/test_compiled_core_model.py on what the feature engines run"""
    from tests.test_compiled_core_model import test_census
    test_census(True)
    assert [p.name for p in C.program().probes if p.two] == ["tell/two_in_order"]
    assert {p.name for p in C.program(True).probes} == {p.name for p in C.program().probes if not p.two}


@pytest.mark.parametrize("variant", C.VARIANT_NAMES)
def test_witness_tells_the_variant_from_a_plain_engine(built, variant):
    """what test_feature_variant takes as the proof that the engine is the variant does not hold on an engine with the
    same actors, tables and tells and without the feature"""
    prog = C.program(True)
    v = C.variants(prog)[variant]
    w = C.workload(prog, 3, bucket_actors=32)
    eng = GpuEngine(config(w))
    try:
        w.apply_to(eng, stage_tells=False)
        assert not C.is_variant(eng, v.witness), (variant, v.witness)
    finally:
        eng.close()


@pytest.mark.parametrize("variant", C.VARIANT_NAMES)
def test_feature_variant(built, pipeline, variant):
    """the single-tell part with the feature switched on and not used: the copy of the rule that variant compiles"""
    v, prog, w, sm, (wm, am, km, im), cr = variant_reference(variant)
    eng = GpuEngine(config(w))
    try:
        w.apply_to(eng, stage_tells=False)
        # the engine is that variant: it answers the witness call as only an engine with the feature does (the info
        # calls answer zeros on any engine, agx_listing_info apart)
        assert C.is_variant(eng, v.witness), (variant, v.witness, C.witness_text(eng, v.witness))
        if v.host_tag_limit < 0xFF:  # the whole program's host tells carry a tag this engine keeps for itself: all or nothing
            with pytest.raises(AgxError):
                eng.tell(*[C.tells(C.program(True))[j] for j in (0, 2, 1)])
            assert eng.stats().staged == 0
        dst, src, pay = w.tells
        eng.tell(dst, pay, src)
        sg = eng.run()
        sg = {k: getattr(sg, k) for k in COUNT_KEYS}
        wg, ag, kg, ig = C.variant_snapshot(eng, v.infos)
    finally:
        eng.close()
    for k in COUNT_KEYS:
        assert sg[k] == sm[k], f"{variant}: {k} gpu={sg[k]} model={sm[k]}"
    assert np.array_equal(ag, am), np.nonzero(ag != am)[0][:8]
    diff = np.nonzero((wg != wm).any(axis=1))[0]
    assert diff.size == 0, (f"{variant}: state differs at {diff[:8]} ({[C.case_of(int(a)) for a in diff[:4]]}) "
                            f"gpu={[[hex(int(x)) for x in r] for r in wg[diff[:3]]]} "
                            f"model={[[hex(int(x)) for x in r] for r in wm[diff[:3]]]}")
    assert np.array_equal(kg, km), np.nonzero(kg != km)[0][:8]
    for i in v.infos:  # the feature never fired, on either side
        for k in set(ig[i]) & set(im[i]):
            assert ig[i][k] == im[i][k], (variant, i, k, ig[i][k], im[i][k])
        assert all(ig[i][k] == 0 for k in v.infos[i]), (variant, i, ig[i])
    # the core model's fold: every actor but those that were sent a message tag this engine keeps for itself (their
    # envelopes also count otherwise there, so the fold's counters hold only where there are none)
    skip = set(cr["reserved"])
    assert len(skip) < C.N // 8
    assert_core(dict(cr, counts={}) if skip else cr, sg, wg, ag, kg, variant, skip)
