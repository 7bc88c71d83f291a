"""TEST INFRASTRUCTURE ONLY.  The seeded LWWMap delta-replication runs that tests/test_gpu_lwwmap_delta.py puts
through the engine, with what each claims to exercise (a key of LwwDeltaModel.census, or a predicate on the
model); tests/test_lwwmap_delta_model.py asserts every claim on the model run, without a GPU."""
from __future__ import annotations

import json
import pathlib

import numpy as np

from akka_amd import workloads as wl
from akka_amd.engine import DELTA_WRITE, Kind, Op
from tests import lwwmap_delta_model as D

GOLD = pathlib.Path(__file__).resolve().parent / "golden"
KATS = json.loads((GOLD / "lwwmap_delta_kats.json").read_text())
W = D.DELTA_WORDS
NO_SENDER = 0xFFFFFFFF


def _w(n, **kw):
    kw.setdefault("bucket_actors", 32)
    return wl.crdt_lwwmap_delta(n, **kw)


def ring_fill(n_ops: int) -> wl.Workload:
    """One key of 8 replicas, each with `n_ops` unsent seqNrs before its first tick: 30 puts of key 5 (they
    coalesce into one op), then puts alternating between keys 6 and 7 (one op each), so a group over all 64
    seqNrs has 35 ops, below max-delta-size 50, and is told."""
    n = 8
    ops = [Op.put(5, 100 + i) for i in range(30)] + [Op.put(6 + (i & 1), 200 + i) for i in range(n_ops - 30)]
    ids = np.arange(n, dtype=np.uint32)
    dst = np.concatenate([np.repeat(ids, n_ops), ids])
    pay = np.concatenate([np.tile(np.array(ops, np.uint32), n), np.full(n, Op.make(Op.DELTA_TICK, 3), np.uint32)])
    return wl.Workload(f"lwwmap_ring_{n_ops}", n, W, 4, 5, 0, [(0, n, Kind.LWWMAP, None)], gossip=(1, 7), lwwmap=("default", 0),
                       lwwmap_delta=50, tells=(dst, np.full(dst.size, NO_SENDER, np.uint32), pay), bucket_actors=32)


# name -> (workload factory, engine config extras, claims)
# a claim is a census key that must be > 0, or ("name", predicate on the model)
CASES = {}
for _n in (8, 9, 20, 72):
    CASES[f"pop_{_n}"] = (lambda n=_n: _w(n, rounds=6, write=True, ops_per_replica=3, gossip_rounds=3), {},
                          ["applied_props", "coalesced_puts"] if _n >= 20 else ["applied_props"])
CASES["pop_4096"] = (lambda: _w(4096, rounds=3, write=True, ops_per_replica=2, gossip_rounds=1, bucket_actors=512), {},
                     ["applied_props", "uncoalesced_groups"])
for _t, _c in ((5, 0), (1, 0), (2, 6)):
    _claims = ["applied_props", "uncoalesced_groups"]
    if (_t, _c) != (5, 0):
        _claims += ["queued_props"]
    if _c:
        _claims += ["dropped_props", "skipped_props"]
    CASES[f"caps_T{_t}_C{_c}"] = (lambda t=_t, c=_c: _w(77, rounds=8, write=True, ops_per_replica=3, gossip_rounds=6,
                                                      throughput=t, capacity=c), {}, _claims)
for _m in (1, 2, 50):
    CASES[f"max_delta_{_m}"] = (lambda m=_m: _w(72, rounds=5, write=False, ops_per_replica=9, max_delta_size=m), {},
                                ["placeholders"] if _m < 50 else ["uncoalesced_groups", "coalesced_puts"])
# max-delta-size 1 with writer ticks: a tick that finds one unsent seqNr for a node tells it (a single seqNr is never
# a placeholder), one that finds two or more voids the group
CASES["max_delta_1_writers"] = (lambda: _w(40, rounds=8, write=True, gossip_rounds=3, max_delta_size=1), {},
                                ["applied_props", "placeholders",
                                 ("every told group is one seqNr", lambda m: m.census["single_seq_groups"] > 0 and
                                  m.census["single_seq_groups"] == m.census["groups"] - m.census["placeholders"])])
for _ba in (32, 512, 2048):
    CASES[f"bucket_{_ba}"] = (lambda ba=_ba: _w(600, rounds=4, write=True, gossip_rounds=2, bucket_actors=ba), {}, ["applied_props"])
CASES["skew"] = (lambda: _w(800, rounds=5, write=True, gossip_rounds=5, fanout=2, bucket_actors=2048), {},
                 ["applied_props", ("a bucket inbox over one tile of 2048", lambda m: m.max_bucket_inbox(2048) > 2048)])
CASES["multipass"] = (lambda: _w(8 * 40 + 3, rounds=6, write=True, ops_per_replica=2, gossip_rounds=2), {}, ["applied_props"])
CASES["reverse_clock"] = (lambda: _w(40, rounds=6, write=True, ops_per_replica=3, gossip_rounds=2, clock="reverse", base=5), {},
                          ["applied_props", ("negative timestamps", lambda m: min(r[2] for x in m.maps for r in x.values.values()) < -5)])
CASES["base_2_41"] = (lambda: _w(40, rounds=6, write=True, ops_per_replica=3, gossip_rounds=2, base=(1 << 41) + 12345), {},
                      ["applied_props", ("timestamps above 2^40 with a non-zero low half",
                                         lambda m: all(r[2] > (1 << 40) and r[2] & 0xFFFFFFFF for x in m.maps for r in x.values.values()))])
CASES["ring_64"] = (lambda: ring_fill(64), {},
                    ["applied_props", "coalesced_puts", ("no capacity error", lambda m: not m.capacity_error),
                     ("a group over 64 seqNrs was told", lambda m: all(m.dv[a][0] == 64 for a in range(1, 8)))])


def model_run(name, drive=None):
    factory, _, _ = CASES[name]
    w = factory()
    m = D.LwwDeltaModel(**w.engine_kwargs())
    w.apply_to(m)
    st = (drive or (lambda t: t.run()))(m)
    return w, m, st


def assert_claims(name, model):
    for c in CASES[name][2]:
        if isinstance(c, str):
            assert model.census[c] > 0, (name, c, model.census)
        else:
            assert c[1](model), (name, c[0], model.census)


def run_engine_script(case, target) -> list:
    """One engine script of the KAT file through `target` (a GpuEngine or an LwwDeltaModel over case["replicas"]
    actors, nothing registered yet): one run per step, every `expect` checked on the decoded state.  Returns
    the state words after every run, for a comparison between two targets."""
    n = case["replicas"]
    target.register_range(0, n, Kind.LWWMAP, None)
    target.set_gossip(1, 1)
    target.set_lwwmap("default", 0)
    target.set_lwwmap_delta(50)
    trace = []
    for i, st in enumerate(case["script"]):
        where = f"{case['name']} step {i} {st}"
        if "expect" in st:
            words, _ = target.read_state()
            from akka_amd.ddata import LWWMap
            got = LWWMap.from_words(words[st["expect"]]).entries
            assert got == {int(k): v for k, v in st["entries"].items()}, (where, got)
            continue
        if "tell" in st:
            dst = [t[0] for t in st["tell"]]
            pay = [Op.put(t[2], t[3]) if t[1] == "put" else Op.make(Op.REMOVE, t[2]) for t in st["tell"]]
            target.tell(dst, pay)
        elif "tick" in st:
            target.tell([st["tick"]], [Op.make(Op.DELTA_TICK, st["k"])])
        elif "gossip" in st:
            target.tell([st["gossip"]], [Op.make(Op.GOSSIP, 0)])
        else:
            raise AssertionError(where)
        stats = target.run()
        stats = stats if isinstance(stats, dict) else {k: getattr(stats, k) for k in ("unhandled", "in_flight", "dead_letters")}
        assert stats["unhandled"] == 0 and stats["in_flight"] == 0 and stats["dead_letters"] == 0, (where, stats)
        trace.append(target.read_state()[0][:, :W].copy())
    return trace
