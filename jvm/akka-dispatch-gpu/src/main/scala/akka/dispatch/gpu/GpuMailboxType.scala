/*
 * mailbox-type = "akka.dispatch.gpu.GpuMailboxType": Mailboxes.lookupConfigurator instantiates
 * it reflectively with the (ActorSystem.Settings, Config) constructor (akka-actor/src/main/
 * scala/akka/dispatch/Mailboxes.scala:222-236); MailboxType.create (Mailbox.scala:638-640)
 * registers the owner as one fixed-layout actor of the dispatcher's engine, bound to the engine
 * mailbox class of this mailbox type's capacity -- so bounded and unbounded GPU mailboxes coexist
 * on one dispatcher, each actor with its own (Mailboxes.scala:204-260, ActorMailboxSpec.scala:245-450).
 *
 * Two mailbox types, like the reference's UnboundedMailbox / BoundedMailbox (Mailbox.scala:647-720):
 * GpuMailboxType (ProducesMessageQueue[GpuMessageQueue], UnboundedMessageQueueSemantics) and
 * GpuBoundedMailboxType (ProducesMessageQueue[GpuBoundedMessageQueue], BoundedMessageQueueSemantics,
 * mailbox-capacity > 0) -- Mailboxes.getMailboxType checks an actor's RequiresMessageQueue against
 * the type's marker (Mailboxes.scala:122-135,164-175), so an actor that requires bounded semantics
 * must be given the bounded type.  A GpuMailboxType with mailbox-capacity > 0 still tail-drops at
 * that capacity and its queues are GpuBoundedMessageQueue at run time.
 *
 * Priority and control-aware mailboxes (Mailbox.scala:726-816, 867-1025): GpuPriorityMailboxType
 * (gpu.priority-by-tag) and GpuControlAwareMailboxType (gpu.control-tags) bind a priority table by
 * message tag (payload >>> 24) to their engine mailbox class (agx_set_mailbox_priority): lower first,
 * FIFO among equal priorities, admission by arrival position at mailbox-capacity.  The reference's
 * priority mailboxes take a Comparator[Envelope] from a user subclass; a GPU actor's messages are
 * fixed-layout payloads, so the comparator is given as data in the mailbox's config block.
 */
package akka.dispatch.gpu

import java.util.concurrent.atomic.AtomicInteger


import com.typesafe.config.Config

import scala.concurrent.duration.Duration

import akka.actor.{ ActorRef, ActorSystem, DeadLetter }
import akka.dispatch._

/** The fixed-layout message of a GPU actor: one u32 payload word (the sender travels in the Envelope). */
final case class GpuTell(payload: Int)

abstract class GpuMailboxTypeBase(settings: ActorSystem.Settings, config: Config) extends MailboxType {

  private val dispatcherId = config.getString("gpu.dispatcher")
  private val kind: Int = config.getString("gpu.behavior") match {
    case "counter"    => Agx.KindCounter
    case "ring"       => Agx.KindRing
    case "fanout"     => Agx.KindFanout
    case "forward-rr" => Agx.KindForwardRR
    case "stop-after" => Agx.KindStopAfter
    case "ping-pong"  => Agx.KindPingPong
    case "even"       => Agx.KindEven
    case "gcounter"   => Agx.KindGCounter
    case "pncounter"  => Agx.KindPNCounter
    case "orset"      => Agx.KindORSet
    case other        => throw new akka.ConfigurationException(s"Unknown GPU behavior [$other] in mailbox config")
  }

  /** BoundedMailbox's keys (Mailbox.scala:699-720): mailbox-capacity, mailbox-push-timeout-time.
   *  The GPU mailbox tail-drops at capacity (pushTimeOut 0, AbstractBoundedNodeQueue.java:92-113);
   *  a positive push timeout would block the sender, which a superstep cannot do. */
  protected val capacity: Int = if (config.hasPath("mailbox-capacity")) config.getInt("mailbox-capacity") else 0
  if (capacity < 0) throw new IllegalArgumentException("The capacity for GpuMailboxType can not be negative")
  if (capacity > 0 && config.hasPath("mailbox-push-timeout-time") &&
      config.getDuration("mailbox-push-timeout-time").toNanos != 0L)
    throw new akka.ConfigurationException(
      "GpuMailboxType is a non-blocking bounded mailbox: mailbox-push-timeout-time must be 0")

  /** The class's priority by message tag (256 bytes, lower first), or null: FIFO. */
  protected def priorityTable: Array[Byte] = null

  override def create(owner: Option[ActorRef], system: Option[ActorSystem]): MessageQueue = {
    val engine = GpuEngine.forDispatcher(dispatcherId)
    val id = owner match {
      case Some(ref) => engine.register(ref, kind, Array.fill(engine.stateWords)(0L), capacity, priorityTable)
      case None      => Agx.NoSender // the dummy queue of a top-level actor under construction
    }
    val q: GpuQueue =
      if (capacity > 0) new GpuBoundedMessageQueue(id, engine, system, capacity)
      else new GpuMessageQueue(id, engine, system)
    q
  }
}

/** mailbox-type = "akka.dispatch.gpu.GpuMailboxType": unbounded semantics (UnboundedMailbox). */
class GpuMailboxType(settings: ActorSystem.Settings, config: Config)
    extends GpuMailboxTypeBase(settings, config)
    with ProducesMessageQueue[GpuMessageQueue]

/** mailbox-type = "akka.dispatch.gpu.GpuBoundedMailboxType": BoundedMailbox(mailbox-capacity, 0)
 *  semantics (Mailbox.scala:699-720), tail-drop to dead letters at the capacity. */
class GpuBoundedMailboxType(settings: ActorSystem.Settings, config: Config)
    extends GpuMailboxTypeBase(settings, config)
    with ProducesMessageQueue[GpuBoundedMessageQueue] {
  if (capacity <= 0)
    throw new IllegalArgumentException("The capacity for GpuBoundedMailboxType must be positive (mailbox-capacity)")
}

/** mailbox-type = "akka.dispatch.gpu.GpuControlAwareMailboxType": Unbounded / BoundedControlAwareMailbox
 *  (Mailbox.scala:867-1025) -- messages whose tag is listed in `gpu.control-tags = [..]` (the
 *  ControlMessage marker of a fixed-layout payload) are handed out before all others, each group
 *  FIFO; mailbox-capacity > 0 bounds both together. */
class GpuControlAwareMailboxType(settings: ActorSystem.Settings, config: Config)
    extends GpuMailboxTypeBase(settings, config)
    with ProducesMessageQueue[GpuMessageQueue] {
  private val table: Array[Byte] = {
    val t = Array.fill[Byte](256)(1)
    if (config.hasPath("gpu.control-tags")) {
      val it = config.getIntList("gpu.control-tags").iterator()
      while (it.hasNext) {
        val tag = it.next().intValue
        if (tag < 0 || tag > 255) throw new akka.ConfigurationException(s"gpu.control-tags: [$tag] is not a message tag (0..255)")
        t(tag) = 0
      }
    }
    t
  }
  override protected def priorityTable: Array[Byte] = table
}

/** mailbox-type = "akka.dispatch.gpu.GpuPriorityMailboxType": Unbounded / BoundedStablePriorityMailbox
 *  (Mailbox.scala:779-816; the unstable types' order among equal priorities is unspecified, and the
 *  stable one is a legal instance, :726-766).  `gpu.priority-by-tag { "<tag>" = <Int>, .. }` is the
 *  PriorityGenerator as data: lower is handed out first; tags not listed come after every listed one.
 *  The Ints are replaced by their dense ranks (a priority queue uses only their order), so any Int fits. */
class GpuPriorityMailboxType(settings: ActorSystem.Settings, config: Config)
    extends GpuMailboxTypeBase(settings, config)
    with ProducesMessageQueue[GpuMessageQueue] {
  private val table: Array[Byte] = {
    val given = new java.util.TreeMap[Integer, java.lang.Long]()
    if (config.hasPath("gpu.priority-by-tag")) {
      val it = config.getConfig("gpu.priority-by-tag").entrySet().iterator()
      while (it.hasNext) {
        val e = it.next()
        val tag = e.getKey.replace("\"", "").toInt
        if (tag < 0 || tag > 255) throw new akka.ConfigurationException(s"gpu.priority-by-tag: [$tag] is not a message tag (0..255)")
        given.put(tag, e.getValue.unwrapped().asInstanceOf[Number].longValue)
      }
    }
    val last: Long = if (given.isEmpty) 0L else java.util.Collections.max(given.values()).longValue + 1
    val value = Array.tabulate[Long](256)(t => if (given.containsKey(t)) given.get(t).longValue else last)
    val ranks = value.distinct.sorted.zipWithIndex.toMap
    value.map(v => ranks(v).toByte)
  }
  override protected def priorityTable: Array[Byte] = table
}

/** The device-side mailbox of one actor.  enqueue hands the tell to the engine through the
 *  lock-free tell path (GpuEngine.tell -> agx_tell: the calling thread's own queue, no lock;
 *  AbstractNodeQueue.java:79-82) and submits the dispatcher's pump only when the engine went from
 *  idle to scheduled (Mailbox.setAsScheduled, Mailbox.scala:185-194).  Nothing is ever dequeued on
 *  the JVM (MessageQueue contract, Mailbox.scala:359-390): the messages live in the engine, in its
 *  in-flight count (GpuEngine.stats()(6)), so numberOfMessages is 0 on the JVM side. */
sealed abstract class GpuQueue(val id: Int, engine: GpuEngine, system: Option[ActorSystem]) extends MessageQueue {

  def enqueue(receiver: ActorRef, handle: Envelope): Unit = {
    val payload = handle.message match {
      case GpuTell(p) => p
      case i: Int     => i
      case other =>
        // not in the fixed-layout protocol: deadLetters, like a tell the actor cannot accept
        system.foreach(_.deadLetters ! DeadLetter(other, handle.sender, receiver))
        return
    }
    engine.tell(id, engine.idOf(handle.sender), payload)
  }

  def dequeue(): Envelope = null
  def numberOfMessages: Int = 0
  def hasMessages: Boolean = false
  def cleanUp(owner: ActorRef, deadLetters: MessageQueue): Unit = () // the engine dead-letters them
}

/** A GPU actor's unbounded mailbox. */
final class GpuMessageQueue(id: Int, engine: GpuEngine, system: Option[ActorSystem])
    extends GpuQueue(id, engine, system)
    with UnboundedMessageQueueSemantics

/** A GPU actor's bounded mailbox: admission `p < capacity` on the device, the rest dead letters;
 *  never blocks a sender (pushTimeOut 0, AbstractBoundedNodeQueue.java:92-113). */
final class GpuBoundedMessageQueue(id: Int, engine: GpuEngine, system: Option[ActorSystem], val capacity: Int)
    extends GpuQueue(id, engine, system)
    with BoundedMessageQueueSemantics {
  def pushTimeOut: Duration = Duration.Zero
}
