"""Restatement of OutboundMessageQueue.SendMessage's queue rule for the sender-queue tests
(SURVEY 8 a14), written from the reference's source:

  src/Orleans.Runtime/Messaging/OutboundMessageQueue.cs:54-131   SendMessage
  src/Orleans.Core/Messaging/Message.cs:75-80                    enum Categories { Ping, System, Application }
  src/Orleans.Core/Messaging/Message.cs:293-302                  IsExpired

Two forms: send_queues_loop, a literal per-message loop that appends to one Python list per queue,
and send_queues_np, the same vectorised for the larger sizes.  Both return
(send_status u8[n], queue u32[n], perm u32[n], offsets u32[n_queues + 5]).

Buckets: 0 loopback, 1 ping sender, 2 system sender, 3 + q application sender q, 3 + n_queues the
trailing bucket (everything not queued)."""
import numpy as np

INT32_MIN = -(1 << 31)
TTL_NONE = (1 << 63) - 1
NO_SILO = 0xFFFFFFFF
SEND_QUEUED, SEND_LOOPBACK, SEND_EXPIRED, SEND_NO_SILO, SEND_UNKNOWN_SILO, SEND_THROWS, SEND_HELD = range(7)
ROUTE_OK, ROUTE_SYSTEM_TARGET, ROUTE_MEMBERSHIP = 0, 2, 3
CAT_PING, CAT_SYSTEM, CAT_APPLICATION = 0, 1, 2        # Message.cs:75-80


class MathAbsOverflow(OverflowError):
    """Math.Abs(int.MinValue): 'Negating the minimum value of a twos complement number is invalid.'"""


def math_abs(v: int) -> int:
    if v == INT32_MIN:
        raise MathAbsOverflow()
    return -v if v < 0 else v


def send_one(silo, route_status, category, ttl, silo_hash, n_queues, my_silo):
    """(send_status, bucket) of one message; the checks in the reference's order."""
    trailing = 3 + n_queues
    # not addressed yet (Dispatcher.AddressMessage left it to the slow path): SendMessage is not reached
    if route_status is not None and route_status not in (ROUTE_OK, ROUTE_SYSTEM_TARGET, ROUTE_MEMBERSHIP):
        return SEND_HELD, trailing
    # :65-69  if (msg.IsExpired) { msg.DropExpiredMessage(...); return; }
    # Message.cs:297-300  if (!TimeToLive.HasValue) return false; return TimeToLive <= TimeSpan.Zero;
    if ttl is not None and ttl != TTL_NONE and ttl <= 0:
        return SEND_EXPIRED, trailing
    # :82-87  if (msg.TargetSilo == null) { ... SendRejection(msg, Unrecoverable, ...); return; }
    if silo == NO_SILO:
        return SEND_NO_SILO, trailing
    if silo >= len(silo_hash):
        return SEND_UNKNOWN_SILO, trailing
    # :90-95  if (msg.TargetSilo.Equals(messageCenter.MyAddress)) ... InboundQueue.PostMessage(msg);
    if silo == my_silo:
        return SEND_LOOPBACK, 0
    # :113-129  switch (msg.Category)
    cat = CAT_APPLICATION if category is None else category
    if cat == CAT_PING:                                   # :115-117 pingSender.QueueRequest(msg)
        return SEND_QUEUED, 1
    if cat == CAT_SYSTEM:                                 # :119-121 systemSender.QueueRequest(msg)
        return SEND_QUEUED, 2
    try:                                                  # :123-128 default:
        index = math_abs(int(silo_hash[silo])) % n_queues   # :125
    except MathAbsOverflow:
        return SEND_THROWS, trailing
    return SEND_QUEUED, 3 + index                         # :126 senders[index].Value.QueueRequest(msg)


def send_queues_loop(silo, route_status, category, ttl, silo_hash, n_queues, my_silo):
    n = len(silo)
    B = n_queues + 4
    queues = [[] for _ in range(B)]                       # each sender is a FIFO (SiloMessageSender.QueueRequest)
    st = np.zeros(n, np.uint8)
    q = np.zeros(n, np.uint32)
    for i in range(n):
        s, b = send_one(int(silo[i]), None if route_status is None else int(route_status[i]),
                        None if category is None else int(category[i]), None if ttl is None else int(ttl[i]),
                        silo_hash, n_queues, my_silo)
        st[i], q[i] = s, b
        queues[b].append(i)
    perm = np.array([i for lst in queues for i in lst], dtype=np.uint32)
    offsets = np.zeros(B + 1, np.uint32)
    offsets[1:] = np.cumsum([len(lst) for lst in queues])
    return st, q, perm, offsets


def send_queues_np(silo, route_status, category, ttl, silo_hash, n_queues, my_silo):
    silo = np.asarray(silo, dtype=np.uint32)
    n = len(silo)
    B = n_queues + 4
    trailing = 3 + n_queues
    sh = np.asarray(silo_hash, dtype=np.int64)            # int32 values, widened: abs cannot wrap
    throws_tab = sh == INT32_MIN                          # the INT32_MIN case before any abs
    app_tab = np.where(throws_tab, 0, 3 + np.abs(np.where(throws_tab, 0, sh)) % n_queues)
    st = np.full(n, 255, np.uint8)
    q = np.full(n, trailing, np.uint32)
    todo = np.ones(n, bool)

    def settle(mask, status, bucket=None):
        m = todo & mask
        st[m] = status
        if bucket is not None:
            q[m] = bucket[m] if isinstance(bucket, np.ndarray) else bucket
        todo[m] = False

    if route_status is not None:
        rs = np.asarray(route_status, dtype=np.uint8)
        settle(~np.isin(rs, (ROUTE_OK, ROUTE_SYSTEM_TARGET, ROUTE_MEMBERSHIP)), SEND_HELD)
    if ttl is not None:
        t = np.asarray(ttl, dtype=np.int64)
        settle((t != TTL_NONE) & (t <= 0), SEND_EXPIRED)
    settle(silo == NO_SILO, SEND_NO_SILO)
    settle(silo >= len(sh), SEND_UNKNOWN_SILO)
    settle(silo == my_silo, SEND_LOOPBACK, 0)
    cat = np.full(n, CAT_APPLICATION, np.uint8) if category is None else np.asarray(category, dtype=np.uint8)
    settle(cat == CAT_PING, SEND_QUEUED, 1)
    settle(cat == CAT_SYSTEM, SEND_QUEUED, 2)
    known = np.minimum(silo, len(sh) - 1)
    settle(throws_tab[known], SEND_THROWS)
    settle(np.ones(n, bool), SEND_QUEUED, app_tab[known].astype(np.uint32))
    perm = np.argsort(q, kind="stable").astype(np.uint32)
    offsets = np.zeros(B + 1, np.uint32)
    offsets[1:] = np.cumsum(np.bincount(q, minlength=B))
    return st, q, perm, offsets


def mixed_batch(rng, n, n_silos, my_silo, silo_hash=None):
    """A batch with every status and all three categories (plus other category bytes) present
    when n is a few hundred or more: (silo, route_status, category, ttl)."""
    silo = rng.integers(0, n_silos, size=n).astype(np.uint32)
    silo[rng.random(n) < 0.05] = NO_SILO
    silo[rng.random(n) < 0.05] = n_silos + rng.integers(0, 5)
    silo[rng.random(n) < 0.10] = my_silo
    rs = rng.choice(np.array([0, 0, 0, 0, 0, 2, 3, 1, 4, 5, 6, 7], np.uint8), size=n)
    cat = rng.choice(np.array([2, 2, 2, 2, 0, 1, 7, 255], np.uint8), size=n)
    ttl = rng.integers(1, 1 << 40, size=n).astype(np.int64)
    ttl[rng.random(n) < 0.3] = TTL_NONE
    ttl[rng.random(n) < 0.04] = 0
    ttl[rng.random(n) < 0.04] = -rng.integers(1, 1 << 40)
    return silo, rs, cat, ttl


def hashes_with_edges(rng, n_silos):
    """A synthetic silo-hash table holding INT32_MIN, -1, 0, 1 and INT32_MAX (when it has room)."""
    sh = rng.integers(INT32_MIN, 1 << 31, size=n_silos).astype(np.int32)
    edges = [INT32_MIN, -1, 0, 1, (1 << 31) - 1]
    for k, v in enumerate(edges[:max(0, n_silos - 1)]):
        sh[(k + 1) % n_silos] = v
    return sh
