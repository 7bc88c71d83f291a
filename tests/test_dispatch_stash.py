"""Deque-based mailbox types of the dispatcher layer (akka_amd/dispatch.py): HOCON lookup of the
reference's mailbox ids and FQCNs, the `stash-capacity` key, and the refusal of an unbounded stash."""
import pytest

from akka_amd.config import Config, ConfigurationException
from akka_amd.dispatch import BoundedDequeBasedMailbox, Mailboxes, UnboundedDequeBasedMailbox


def test_lookup_by_reference_ids():
    mbs = Mailboxes(Config.parse_string("""
    akka.actor.default-mailbox { stash-capacity = 16, mailbox-push-timeout-time = 0s }"""))  # (GPU mailboxes never block)
    u = mbs.lookup("unbounded-deque-based")
    assert type(u) is UnboundedDequeBasedMailbox and u.capacity == 0 and u.stash_capacity == 16
    b = mbs.lookup("bounded-deque-based")
    assert type(b) is BoundedDequeBasedMailbox and b.capacity == 1000 and b.stash_capacity == 16


def test_lookup_by_fqcn_and_own_keys():
    mbs = Mailboxes(Config.parse_string("""
    my-stash-mailbox {
      mailbox-type = "akka.dispatch.BoundedDequeBasedMailbox"
      mailbox-capacity = 4
      mailbox-push-timeout-time = 0s
      stash-capacity = 3
    }
    my-deque { mailbox-type = "akka.dispatch.UnboundedDequeBasedMailbox", stash-capacity = 255 }"""))
    b = mbs.lookup("my-stash-mailbox")
    assert (b.capacity, b.stash_capacity) == (4, 3)
    assert mbs.lookup("my-deque").stash_capacity == 255


def test_unbounded_stash_is_refused():
    """the reference's default stash-capacity = -1 (unbounded) has no GPU counterpart"""
    with pytest.raises(ConfigurationException) as e:
        Mailboxes(Config()).lookup("unbounded-deque-based")
    assert "stash-capacity = -1" in str(e.value) and "1..255" in str(e.value)
    for bad in (0, 256):
        with pytest.raises(ConfigurationException):
            UnboundedDequeBasedMailbox(bad)


def test_bounded_deque_push_timeout_refused():
    with pytest.raises(ConfigurationException):
        BoundedDequeBasedMailbox(4, 3, push_timeout_s=1.0)
