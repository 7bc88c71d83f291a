"""Pub-sub topics, without a GPU: the model (tests/topic_model.py, DESIGN.md §2.10 in Python) against the known
answers restated from the reference's spec (tests/golden/topic_kats.json), the inbox-order rule, the documented
same-window differences, conservation after every run, and the premises of the GPU cases."""
import numpy as np
import pytest

from tests import topic_cases as tc
from tests.topic_model import TopicModel


def model_for(w):
    m = TopicModel(**w.engine_kwargs())
    w.apply_to(m)
    return m


def run_script(w, script):
    """the model through the script: (stats, snapshot) after every run, conservation checked"""
    m, out = model_for(w), []
    for st in script(m):
        st = tc.counts(st)
        snap = tc.snapshot(m)
        assert tc.conserved(st, snap["topic_info"]), (len(out), st, snap["topic_info"])
        out.append((st, snap))
    return m, out


@pytest.mark.parametrize("T", tc.KAT_T)
@pytest.mark.parametrize("name", tc.KAT_NAMES)
def test_kat(name, T):
    got = tc.run_kat(name, model_for(tc.node_workload(T)))
    tc.check_kat(name, got)


def test_kats_cite_the_spec():
    for s in tc.KATS["scenarios"]:
        assert "LocalPubSubSpec.scala:" in s["cite"]
    assert len(tc.KATS["scenarios"]) == 3


def test_inbox_order():
    """backlog ++ arrivals ++ host-staged tells ++ publications in (publisher, window index) order"""
    m, out = run_script(tc.order_workload(), tc.order_script)
    # the log after tick 1: publisher 5, then 130's two publications in window order, then 250
    assert out[0][1]["log"] == [[1, 5, tc.payload("Note:2")], [0, 130, tc.payload("Note:1")], [1, 130, tc.payload("Note:3")],
                                [0, 250, tc.payload("Note:4")]]
    assert out[0][0]["in_flight"] == 1 + 12 + 6 + 6 + 12  # the Ping of 7's Poke and the planned deliveries
    got = tc.got_of(out[1][1])
    for a, more in tc.got_of(out[2][1]).items():  # (T = 5: the sixth message of 63 is drained a tick later)
        got[a] = got.get(a, []) + more
    assert got[63] == [63, 8, 2, 1, 3, 4]  # the device tell, the host-staged tell, then the log in order
    assert got[64] == [9, 2, 1, 3, 4]
    assert got[60] == [1, 4] and got[200] == [1, 4] and got[201] == [2, 3]
    assert not any(128 <= a < 192 for a in got)  # bucket 2 has no subscriber
    assert out[2][1]["words"][63][1] == 250  # the sender of a delivery is the publisher
    assert out[2][1]["topic_info"] == dict(published=4, fanned_out=36, no_subscribers=0, host_published=0)


def test_membership_timing_and_documented_differences():
    m, out = run_script(tc.timing_workload(), tc.timing_script)
    got = tc.got_of(out[2][1])
    assert got[20] == [2, 1, 3]     # (the log is in publisher order: 5, 20, 22) subscribe and publish in one window: it receives its own publication, as in Akka
    assert got[21] == [2, 1, 3]     # subscribed by another actor's tick: receives
    assert 22 not in got            # publish then unsubscribe in one window: not received (in Akka it would be)
    assert 70 not in got and 140 not in got
    assert got[10] == [2, 1, 3] and got[141] == [2, 1, 3]
    d0 = out[2][0]["dead_letters"]
    assert out[4][0]["dead_letters"] == d0 + 1 and out[4][1]["alive"][141] == 0  # stopped before draining the delivery
    got = tc.got_of(out[6][1])
    assert sorted(got) == [20, 21, 100, 101, 102] and 10 not in got  # register_services between the two ticks
    assert out[5][1]["topic_info"]["fanned_out"] + 3 - 1 == out[6][1]["topic_info"]["fanned_out"]  # the re-plan
    # a publication without a recipient is not quiescence's business: the run ends, the log waits for its tick
    assert out[7][0]["in_flight"] == 0 and len(out[7][1]["log"]) == 1 and out[7][1]["topic_info"]["no_subscribers"] == 1
    assert sorted(tc.got_of(out[8][1])) == [30, 31] and out[8][1]["topic_info"]["no_subscribers"] == 0
    assert out[8][1]["log"] == []


def test_bounded_mailboxes():
    m, out = run_script(tc.bounded_workload(), tc.bounded_script)
    assert out[0][0]["dead_letters"] == 128  # the third delivery of every subscriber
    assert out[-1][0]["dead_letters"] == 256 and out[-1][0]["in_flight"] == 0
    assert out[-1][1]["topic_info"]["fanned_out"] == 6 * 128


def test_budgets_between_publish_and_delivery():
    m, out = run_script(tc.node_workload(3, n=256, starts=[(60, 11, 0), (200, 1, 1)]), tc.budget_script)
    assert out[0][0]["in_flight"] == 12 and len(out[0][1]["log"]) == 2
    assert out[1][0]["in_flight"] == 0 and out[1][0]["delivered"] == 2 + 12
    assert out[3][0]["in_flight"] == 11 and out[-1][0]["in_flight"] == 0


def test_host_publish():
    m, out = run_script(tc.order_workload(), tc.host_publish_script)
    assert out[0][0]["delivered"] == 12 + 6 and out[0][1]["topic_info"]["host_published"] == 2
    assert out[0][1]["words"][60][1] == 300 and out[0][1]["words"][201][1] == tc.NO_SENDER
    assert [e[2] & 0xFFFFFF for e in out[2][1]["log"]] == [] and tc.got_of(out[2][1])[60] == [3, 4, 5, 6]
    assert out[-1][1]["topic_info"] == dict(published=2, fanned_out=12 * 5 + 6 * 2, no_subscribers=0, host_published=5)


def test_log_capacity():
    w = tc.node_workload(1, n=64, log_capacity=4, starts=[(0, 4, 0)])
    m = model_for(w)
    tc.tells(m, *[(a, f"PubF:{a}") for a in range(10, 14)])
    m.run()
    assert not m.topic_error
    tc.tells(m, *[(a, f"PubF:{a}") for a in range(10, 15)])
    m.run()
    assert m.topic_error


@pytest.mark.parametrize("bucket_actors", [64, 2048])
@pytest.mark.parametrize("seed", tc.MESH_SEEDS)
def test_premises_of_the_gpu_mesh(seed, bucket_actors):
    """each topic_mesh seed used on the GPU fans out, meets topics without subscribers, loses a delivery to a bounded
    mailbox, stays within the log capacity, the listing capacity and one tile per bucket"""
    w = tc.mesh_workload(seed, bucket_actors)
    m = model_for(w)
    dead_deliveries = 0
    for st in tc.mesh_script(w)(m):
        info = m.topic_info()
        assert tc.conserved(tc.counts(st), info)
        dead_deliveries = m.delivery_dead_letters
    assert info["fanned_out"] > 0 and info["no_subscribers"] > 0 and dead_deliveries > 0
    assert not m.topic_error and not m.capacity_error
    assert m.max_bucket_inbox(bucket_actors) <= 2048
    assert np.asarray(m.alive).sum() < m.n  # (actors stop, too)
