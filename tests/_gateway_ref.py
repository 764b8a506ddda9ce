"""Restatement of the gateway's per-message dictionary path for the gateway tests, written from the
reference's source:

  src/Orleans.Runtime/Messaging/Gateway.cs:117-147    RecordOpenedSocket
  src/Orleans.Runtime/Messaging/Gateway.cs:149-169    RecordClosedSocket
  src/Orleans.Runtime/Messaging/Gateway.cs:171-180    TryToReroute
  src/Orleans.Runtime/Messaging/Gateway.cs:182-222    DropDisconnectedClients, DropExpiredRoutingCachedEntries, DropClient
  src/Orleans.Runtime/Messaging/Gateway.cs:229-257    TryDeliverToProxy, QueueRequest
  src/Orleans.Runtime/Messaging/Gateway.cs:265-306    ClientState
  src/Orleans.Runtime/Messaging/Gateway.cs:340-383    ClientsReplyRoutingCache
  src/Orleans.Runtime/Messaging/Gateway.cs:401-475    GatewaySender.Process
  src/Orleans.Runtime/Messaging/GatewayAcceptor.cs:88-141   HandleMessage
  src/Orleans.Runtime/Messaging/OutboundMessageQueue.cs:64-80
  src/Orleans.Core.Abstractions/IDs/GrainId.cs:23     IsClient

Two forms with one interface: Gateway, a literal loop with one ClientState object a client and dicts for `clients`
and `clientRoutes`, and GatewayNp, the same over arrays.  Keys are (n, 3) uint64 rows [n0, n1, type_code_data];
times are int64 ticks passed in (the reference reads DateTime.UtcNow)."""
import numpy as np

import _sendq_ref as S

CAT_SYSTEM_TARGET, CAT_CLIENT, CAT_GEO_CLIENT = 1, 4, 7          # UniqueKey.cs:17-26
I64_MAX = (1 << 63) - 1                                          # DateTime.MaxValue's stand-in (RecordConnection)
TTL_NONE = S.TTL_NONE
NO_SILO = NO_HANDLE = 0xFFFFFFFF
GW_NOT_PROXIED, GW_SEND, GW_PENDING, GW_EXPIRED, GW_GEO_CLIENT = range(5)
GW_NOT_CLIENT = 0xFF
SEND_PROXIED = 7
GWIN_REROUTE, GWIN_DIRECT, GWIN_SYSTEM_TARGET, GWIN_EXPIRED, GWIN_TOO_BUSY, GWIN_GEO_CLIENT = range(6)
DIR_RESPONSE = 1                                                 # Message.Directions.Response

LOOKUP_NAMES = ("handle", "sender", "connected", "since", "pending", "found", "route_silo", "route_time", "route_found")


def keys(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.uint64).reshape(-1, 3))


def cat_of(tcd):
    return int(tcd) >> 56


def is_client(cat):
    """GrainId.IsClient (GrainId.cs:23): Category == Client || Category == GeoClient."""
    return cat == CAT_CLIENT or cat == CAT_GEO_CLIENT


def client_keys(ids, type_data=0):
    """Client GrainIds: n0 = 0, n1 = id, category Client."""
    ids = np.asarray(ids, dtype=np.uint64)
    k = np.zeros((len(ids), 3), np.uint64)
    k[:, 1] = ids
    k[:, 2] = np.uint64((CAT_CLIENT << 56) | type_data)
    return k


def with_cat(k, cat):
    k = keys(k).copy()
    k[:, 2] = (k[:, 2] & np.uint64((1 << 56) - 1)) | np.uint64(cat << 56)
    return k


def _partition(bucket, B):
    perm = np.argsort(bucket, kind="stable").astype(np.uint32)
    offsets = np.zeros(B + 1, np.uint32)
    offsets[1:] = np.cumsum(np.bincount(bucket, minlength=B))
    return perm, offsets


def _expired(ttl, i):
    # Message.cs:297-300  if (!TimeToLive.HasValue) return false; return TimeToLive <= TimeSpan.Zero;
    return ttl is not None and int(ttl[i]) != TTL_NONE and int(ttl[i]) <= 0


class ClientState:                                               # Gateway.cs:265-306
    def __init__(self, cid, handle, sender):
        self.id, self.handle, self.sender = cid, handle, sender  # Id, the host's object, GatewaySenderNumber
        self.connected = False                                   # Socket != null
        self.since = 0                                           # DisconnectedSince
        self.pending = 0                                         # PendingToSend.Count

    def record_disconnection(self, now):                         # :286-293
        if not self.connected:
            return
        self.since = now
        self.connected = False

    def record_connection(self):                                 # :295-299
        self.connected = True
        self.since = I64_MAX

    def ready_to_drop(self, now, timeout):                       # :301-305
        return not self.connected and now - self.since >= timeout


class Gateway:
    """The literal form: one call a batch, one loop iteration a message."""

    def __init__(self, n_senders, client_drop_timeout, route_expiry):
        self.n_senders, self.drop_timeout, self.route_expiry = n_senders, client_drop_timeout, route_expiry
        self.clients = {}                                        # ConcurrentDictionary<GrainId, ClientState>
        self.routes = {}                                         # clientRoutes: GrainId -> (SiloAddress, DateTime)
        self.next_rr = 0                                         # nextGatewaySenderToUseForRoundRobin

    def count(self):
        return len(self.clients), len(self.routes)

    def open(self, ids, handles):
        ids = keys(ids)
        n = len(ids)
        oh, osd = np.full(n, NO_HANDLE, np.uint32), np.full(n, self.n_senders, np.uint32)
        on, op = np.full(n, GW_NOT_CLIENT, np.uint8), np.zeros(n, np.uint32)
        for i in range(n):
            k = tuple(int(x) for x in ids[i])
            if cat_of(k[2]) != CAT_CLIENT:
                continue
            cs = self.clients.get(k)
            if cs is not None:                                   # :123-133
                op[i] = cs.pending                               # QueueRequest(clientState, null): the drain
                cs.pending = 0
                on[i] = 0
            else:                                                # :134-141
                use = self.next_rr % self.n_senders
                self.next_rr += 1
                cs = ClientState(k, int(handles[i]), use)
                self.clients[k] = cs
                on[i] = 1
            cs.record_connection()                               # :142
            oh[i], osd[i] = cs.handle, cs.sender
        return oh, osd, on, op

    def close(self, ids, now, pending_left=None):
        ids = keys(ids)
        found = np.zeros(len(ids), np.uint8)
        for i in range(len(ids)):
            cs = self.clients.get(tuple(int(x) for x in ids[i]))
            if cs is None:                                       # :155 the socket is nobody's
                continue
            found[i] = 1
            if cs.connected and pending_left is not None:        # what the host still holds after a failed drain
                cs.pending = int(pending_left[i])
            cs.record_disconnection(now)                         # :167
        return found

    def drop(self, now, cap=None):
        """(ids sorted, handle, pending, n_out); n_out > cap: nothing changed or listed."""
        due = [cs for cs in self.clients.values() if cs.ready_to_drop(now, self.drop_timeout)]   # :186
        if cap is not None and len(due) > cap:
            return np.zeros((0, 3), np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), len(due)
        due.sort(key=lambda cs: cs.id)
        for cs in due:
            del self.clients[cs.id]                              # :209
        return (keys([cs.id for cs in due]), np.array([cs.handle for cs in due], np.uint32),
                np.array([cs.pending for cs in due], np.uint32), len(due))

    def routes_expire(self, now):
        gone = [k for k, (_, t) in self.routes.items() if now - t >= self.route_expiry]           # :371,:379-382
        for k in gone:
            del self.routes[k]
        return len(gone)

    def lookup(self, ids):
        ids = keys(ids)
        n = len(ids)
        out = [np.full(n, NO_HANDLE, np.uint32), np.full(n, self.n_senders, np.uint32), np.zeros(n, np.uint8),
               np.zeros(n, np.int64), np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.full(n, NO_SILO, np.uint32),
               np.zeros(n, np.int64), np.zeros(n, np.uint8)]
        for i in range(n):
            k = tuple(int(x) for x in ids[i])
            cs = self.clients.get(k)
            if cs is not None:
                for a, v in zip(out[:6], (cs.handle, cs.sender, cs.connected, cs.since, cs.pending, 1)):
                    a[i] = v
            r = self.routes.get(k)
            if r is not None:
                out[6][i], out[7][i], out[8][i] = r[0], r[1], 1
        return tuple(out)

    def deliver_one(self, tk, sk, ssilo, now):
        """TryDeliverToProxy + GatewaySender.Process for one message: (status, handle, sender)."""
        if cat_of(tk[2]) == CAT_GEO_CLIENT:
            return GW_GEO_CLIENT, NO_HANDLE, self.n_senders
        cs = self.clients.get(tk)                                # :235
        if cs is None or cat_of(tk[2]) != CAT_CLIENT:
            return GW_NOT_PROXIED, NO_HANDLE, self.n_senders     # :236 return false
        if sk is not None and cat_of(sk[2]) == CAT_CLIENT:       # :241 (a geo-client sender: C#'s)
            self.routes[sk] = (ssilo, now)                       # :243, :352-356 AddOrUpdate
        # :248 QueueRequest(client, msg) -> Process (:401-475): the client is there (:408 cannot miss)
        if cs.connected:
            return GW_SEND, cs.handle, cs.sender                 # :431- sends on the socket
        cs.pending += 1                                          # :424-429 PendingToSend.Enqueue
        return GW_PENDING, cs.handle, cs.sender

    def deliver(self, target, sending, sending_silo, now, ttl=None):
        target = keys(target)
        n = len(target)
        sending = None if sending is None else keys(sending)
        st, hd = np.zeros(n, np.uint8), np.full(n, NO_HANDLE, np.uint32)
        sd = np.full(n, self.n_senders, np.uint32)
        for i in range(n):
            if _expired(ttl, i):                                 # OutboundMessageQueue.cs:65-69, before :77
                st[i] = GW_EXPIRED
                continue
            sk = None if sending is None else tuple(int(x) for x in sending[i])
            ss = NO_SILO if sending_silo is None else int(sending_silo[i])
            st[i], hd[i], sd[i] = self.deliver_one(tuple(int(x) for x in target[i]), sk, ss, now)
        perm, offsets = _partition(sd, self.n_senders + 1)       # each sender a FIFO; the rest trails
        return st, hd, sd, perm, offsets

    def send_queues(self, target, sending, sending_silo, silo, now, route_status, category, ttl, silo_hash, n_queues,
                    my_silo):
        """OutboundMessageQueue.SendMessage with :77 in place: the loop of _sendq_ref with the proxy check."""
        target = keys(target)
        n = len(target)
        sending = None if sending is None else keys(sending)
        st, q, hd = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.full(n, NO_HANDLE, np.uint32)
        for i in range(n):
            rs = None if route_status is None else int(route_status[i])
            s, b = S.send_one(int(silo[i]), rs, None if category is None else int(category[i]),
                              None if ttl is None else int(ttl[i]), silo_hash, n_queues, my_silo)
            if s not in (S.SEND_HELD, S.SEND_EXPIRED):           # :77 runs after :58-69
                sk = None if sending is None else tuple(int(x) for x in sending[i])
                ss = NO_SILO if sending_silo is None else int(sending_silo[i])
                g, h, sender = self.deliver_one(tuple(int(x) for x in target[i]), sk, ss, now)
                if g in (GW_SEND, GW_PENDING):
                    s, b, hd[i] = SEND_PROXIED, n_queues + 4 + sender, h
            st[i], q[i] = s, b
        perm, offsets = _partition(q, n_queues + 4 + self.n_senders)
        return st, q, hd, perm, offsets

    def ingress(self, target, sending, direction, ttl, overloaded, my_silo):
        target = keys(target)
        n = len(target)
        sending = None if sending is None else keys(sending)
        st, silo, idx = np.zeros(n, np.uint8), np.full(n, NO_SILO, np.uint32), []
        for i in range(n):
            if _expired(ttl, i):                                 # GatewayAcceptor.cs:91
                st[i] = GWIN_EXPIRED
                continue
            if overloaded:                                       # :106-114
                st[i] = GWIN_TOO_BUSY
                continue
            tk = tuple(int(x) for x in target[i])
            tc = cat_of(tk[2])
            d = 0 if direction is None or int(direction[i]) == 0xFF else int(direction[i])
            gateway = None
            # Gateway.cs:174-179 TryToReroute
            if sending is not None and is_client(cat_of(sending[i][2])) and is_client(tc) and d == DIR_RESPONSE:
                if tc == CAT_GEO_CLIENT:
                    st[i] = GWIN_GEO_CLIENT                      # the lookup needs the KeyExt: C#'s
                    continue
                r = self.routes.get(tk)
                if r is not None and r[0] != NO_SILO:            # a route holding null reroutes
                    gateway = r[0]
            if gateway is None:                                  # :119-134
                if tc == CAT_SYSTEM_TARGET:
                    st[i], silo[i] = GWIN_SYSTEM_TARGET, my_silo
                else:
                    st[i] = GWIN_REROUTE
                    idx.append(i)
            else:                                                # :135-140
                st[i], silo[i] = GWIN_DIRECT, gateway
        idx = np.array(idx, np.uint32)
        return st, silo, idx, target[idx.astype(np.int64)]


class GatewayNp:
    """The same over arrays: state is the clients' and the routes' keys with their value columns."""

    def __init__(self, n_senders, client_drop_timeout, route_expiry):
        self.n_senders, self.drop_timeout, self.route_expiry = n_senders, client_drop_timeout, route_expiry
        self.ck = np.zeros((0, 3), np.uint64)
        self.c = {"handle": np.zeros(0, np.uint32), "sender": np.zeros(0, np.uint32), "connected": np.zeros(0, bool),
                  "since": np.zeros(0, np.int64), "pending": np.zeros(0, np.uint32)}
        self.rk = np.zeros((0, 3), np.uint64)
        self.r = {"silo": np.zeros(0, np.uint32), "time": np.zeros(0, np.int64)}
        self.next_rr = 0

    def count(self):
        return len(self.ck), len(self.rk)

    @staticmethod
    def _match(table_keys, batch):
        """Row of each batch key in table_keys (-1 absent), and the index of each key's first occurrence in the batch."""
        if len(batch) == 0:
            return np.zeros(0, np.int64), np.zeros(0, np.int64), None
        both = np.concatenate([table_keys, batch])
        _, first, inv = np.unique(both, axis=0, return_index=True, return_inverse=True)
        m = len(table_keys)
        row = first[inv.reshape(-1)[m:]]
        row = np.where(row < m, row, -1)
        _, bfirst, binv = np.unique(batch, axis=0, return_index=True, return_inverse=True)
        return row, bfirst[binv.reshape(-1)], None

    def open(self, ids, handles):
        ids, handles = keys(ids), np.asarray(handles, dtype=np.uint32)
        n = len(ids)
        oh, osd = np.full(n, NO_HANDLE, np.uint32), np.full(n, self.n_senders, np.uint32)
        on, op = np.full(n, GW_NOT_CLIENT, np.uint8), np.zeros(n, np.uint32)
        ok = (ids[:, 2] >> np.uint64(56)) == CAT_CLIENT
        idx = np.flatnonzero(ok)
        if len(idx) == 0:
            return oh, osd, on, op
        row, first_in_batch, _ = self._match(self.ck, ids[idx])
        is_first = first_in_batch == np.arange(len(idx))          # the first of the id among the batch's new ones
        new = (row < 0) & is_first
        rank = np.cumsum(new) - 1
        # existing clients: the first occurrence drains, every occurrence reconnects
        ex = row >= 0
        first_of_row = np.zeros(len(idx), bool)
        if ex.any():
            _, f = np.unique(row[ex], return_index=True)
            first_of_row[np.flatnonzero(ex)[f]] = True
        op[idx[first_of_row]] = self.c["pending"][row[first_of_row]]
        self.c["pending"][row[ex]] = 0
        self.c["connected"][row[ex]] = True
        self.c["since"][row[ex]] = I64_MAX
        # new clients
        base = len(self.ck)
        nn = int(new.sum())
        senders = ((self.next_rr + rank[new]) % self.n_senders).astype(np.uint32)
        self.next_rr += nn
        self.ck = np.concatenate([self.ck, ids[idx[new]]])
        for name, vals in (("handle", handles[idx[new]]), ("sender", senders), ("connected", np.ones(nn, bool)),
                           ("since", np.full(nn, I64_MAX, np.int64)), ("pending", np.zeros(nn, np.uint32))):
            self.c[name] = np.concatenate([self.c[name], vals])
        # rows of the batch's new ids, by first occurrence
        new_pos = np.flatnonzero(new)
        row_new = np.full(len(idx), -1, np.int64)
        row_new[new_pos] = base + np.arange(nn)
        final = np.where(ex, row, row_new[first_in_batch])
        oh[idx], osd[idx] = self.c["handle"][final], self.c["sender"][final]
        on[idx] = new.astype(np.uint8)
        return oh, osd, on, op

    def close(self, ids, now, pending_left=None):
        ids = keys(ids)
        row, first_in_batch, _ = self._match(self.ck, ids)
        found = (row >= 0).astype(np.uint8)
        act = (row >= 0) & (first_in_batch == np.arange(len(ids)))
        act[act] = self.c["connected"][row[act]]
        r = row[act]
        if pending_left is not None:
            self.c["pending"][r] = np.asarray(pending_left, dtype=np.uint32)[act]
        self.c["since"][r] = now
        self.c["connected"][r] = False
        return found

    def drop(self, now, cap=None):
        due = ~self.c["connected"] & (now - np.where(self.c["connected"], 0, self.c["since"]) >= self.drop_timeout)
        k = int(due.sum())
        if cap is not None and k > cap:
            return np.zeros((0, 3), np.uint64), np.zeros(0, np.uint32), np.zeros(0, np.uint32), k
        ids, hd, pd = self.ck[due], self.c["handle"][due], self.c["pending"][due]
        o = np.lexsort((ids[:, 2], ids[:, 1], ids[:, 0]))
        self.ck = self.ck[~due]
        for name in self.c:
            self.c[name] = self.c[name][~due]
        return ids[o], hd[o], pd[o], k

    def routes_expire(self, now):
        gone = now - self.r["time"] >= self.route_expiry
        self.rk = self.rk[~gone]
        for name in self.r:
            self.r[name] = self.r[name][~gone]
        return int(gone.sum())

    def lookup(self, ids):
        ids = keys(ids)
        n = len(ids)
        row, _, _ = self._match(self.ck, ids)
        f = row >= 0
        out = [np.full(n, NO_HANDLE, np.uint32), np.full(n, self.n_senders, np.uint32), np.zeros(n, np.uint8),
               np.zeros(n, np.int64), np.zeros(n, np.uint32), f.astype(np.uint8), np.full(n, NO_SILO, np.uint32),
               np.zeros(n, np.int64), None]
        for a, name in zip(out[:5], ("handle", "sender", "connected", "since", "pending")):
            a[f] = self.c[name][row[f]]
        rrow, _, _ = self._match(self.rk, ids)
        g = rrow >= 0
        out[6][g], out[7][g], out[8] = self.r["silo"][rrow[g]], self.r["time"][rrow[g]], g.astype(np.uint8)
        return tuple(out)

    def _proxy(self, target, sending, sending_silo, now, consider):
        """TryDeliverToProxy for the messages in `consider`: (found, row)."""
        n = len(target)
        tc = target[:, 2] >> np.uint64(56)
        row, _, _ = self._match(self.ck, target)
        found = consider & (tc == CAT_CLIENT) & (row >= 0)
        np.add.at(self.c["pending"], row[found & ~self.c["connected"][np.maximum(row, 0)]], 1)
        if sending is not None:
            rec = found & ((sending[:, 2] >> np.uint64(56)) == CAT_CLIENT)
            ri = np.flatnonzero(rec)
            if len(ri):
                ss = np.full(n, NO_SILO, np.uint32) if sending_silo is None else np.asarray(sending_silo, np.uint32)
                # the last message of each grain stands
                rev = ri[::-1]
                _, f = np.unique(sending[rev], axis=0, return_index=True)
                last = rev[f]
                rrow, _, _ = self._match(self.rk, sending[last])
                old = rrow >= 0
                self.r["silo"][rrow[old]] = ss[last[old]]
                self.r["time"][rrow[old]] = now
                self.rk = np.concatenate([self.rk, sending[last[~old]]])
                self.r["silo"] = np.concatenate([self.r["silo"], ss[last[~old]]])
                self.r["time"] = np.concatenate([self.r["time"], np.full(int((~old).sum()), now, np.int64)])
        return found, row

    def deliver(self, target, sending, sending_silo, now, ttl=None):
        target = keys(target)
        n = len(target)
        sending = None if sending is None else keys(sending)
        exp = np.zeros(n, bool)
        if ttl is not None:
            t = np.asarray(ttl, dtype=np.int64)
            exp = (t != TTL_NONE) & (t <= 0)
        was_connected = self.c["connected"].copy()
        found, row = self._proxy(target, sending, sending_silo, now, ~exp)
        st = np.full(n, GW_NOT_PROXIED, np.uint8)
        st[~exp & ((target[:, 2] >> np.uint64(56)) == CAT_GEO_CLIENT)] = GW_GEO_CLIENT
        st[exp] = GW_EXPIRED
        st[found] = np.where(was_connected[row[found]], GW_SEND, GW_PENDING)
        hd, sd = np.full(n, NO_HANDLE, np.uint32), np.full(n, self.n_senders, np.uint32)
        hd[found], sd[found] = self.c["handle"][row[found]], self.c["sender"][row[found]]
        perm, offsets = _partition(sd, self.n_senders + 1)
        return st, hd, sd, perm, offsets

    def send_queues(self, target, sending, sending_silo, silo, now, route_status, category, ttl, silo_hash, n_queues,
                    my_silo):
        target = keys(target)
        sending = None if sending is None else keys(sending)
        st, q, _, _ = S.send_queues_np(silo, route_status, category, ttl, silo_hash, n_queues, my_silo)
        found, row = self._proxy(target, sending, sending_silo, now, ~np.isin(st, (S.SEND_HELD, S.SEND_EXPIRED)))
        hd = np.full(len(target), NO_HANDLE, np.uint32)
        st[found], hd[found] = SEND_PROXIED, self.c["handle"][row[found]]
        q[found] = n_queues + 4 + self.c["sender"][row[found]]
        perm, offsets = _partition(q, n_queues + 4 + self.n_senders)
        return st, q, hd, perm, offsets

    def ingress(self, target, sending, direction, ttl, overloaded, my_silo):
        target = keys(target)
        n = len(target)
        tc = target[:, 2] >> np.uint64(56)
        exp = np.zeros(n, bool)
        if ttl is not None:
            t = np.asarray(ttl, dtype=np.int64)
            exp = (t != TTL_NONE) & (t <= 0)
        st, silo = np.full(n, GWIN_REROUTE, np.uint8), np.full(n, NO_SILO, np.uint32)
        st[tc == CAT_SYSTEM_TARGET] = GWIN_SYSTEM_TARGET
        d = np.zeros(n, np.uint8) if direction is None else np.asarray(direction, dtype=np.uint8).copy()
        d[d == 0xFF] = 0
        if sending is not None:
            sc = keys(sending)[:, 2] >> np.uint64(56)
            both = (d == DIR_RESPONSE) & np.isin(sc, (CAT_CLIENT, CAT_GEO_CLIENT)) & np.isin(tc, (CAT_CLIENT, CAT_GEO_CLIENT))
            st[both & (tc == CAT_GEO_CLIENT)] = GWIN_GEO_CLIENT
            rrow, _, _ = self._match(self.rk, target)
            direct = both & (tc == CAT_CLIENT) & (rrow >= 0)
            direct[direct] = self.r["silo"][rrow[direct]] != NO_SILO
            st[direct], silo[direct] = GWIN_DIRECT, self.r["silo"][rrow[direct]]
        if overloaded:
            st[:] = GWIN_TOO_BUSY
        st[exp] = GWIN_EXPIRED
        silo[st == GWIN_SYSTEM_TARGET] = my_silo
        silo[~np.isin(st, (GWIN_DIRECT, GWIN_SYSTEM_TARGET))] = NO_SILO
        idx = np.flatnonzero(st == GWIN_REROUTE).astype(np.uint32)
        return st, silo, idx, target[idx.astype(np.int64)]


def lifecycle(rng, n_clients=40, n=600, n_senders=3):
    """One seed's mixed lifecycle as a list of (call, args): open / deliver / close / deliver / drop / reopen /
    expire / ingress, with every deliver, send and ingress status present (asserted by the tests through
    `cover`)."""
    ids = client_keys(rng.choice(1 << 20, n_clients, replace=False) + 1)
    extra = client_keys(np.arange(n_clients) + (1 << 21))         # never opened
    grains = keys(np.c_[np.zeros(n, np.uint64), rng.integers(1, 1 << 30, n).astype(np.uint64),
                        np.full(n, (3 << 56) | 77, np.uint64)])

    def msgs(now):
        pool = np.concatenate([ids, ids, extra[:8], grains[:64], with_cat(ids[:12], CAT_GEO_CLIENT),
                               with_cat(grains[:4], CAT_SYSTEM_TARGET)])
        target = pool[rng.integers(0, len(pool), n)]
        spool = np.concatenate([ids[:12], extra[:6], grains[:32], with_cat(extra[:3], CAT_GEO_CLIENT)])
        sending = spool[rng.integers(0, len(spool), n)]
        ssilo = rng.integers(0, 8, n).astype(np.uint32)
        ssilo[rng.random(n) < 0.2] = NO_SILO
        ttl = rng.integers(1, 1 << 40, n).astype(np.int64)
        ttl[rng.random(n) < 0.3] = TTL_NONE
        ttl[rng.random(n) < 0.05] = 0
        ttl[rng.random(n) < 0.05] = -5
        return target, sending, ssilo, now, ttl

    def ing():
        t, s, _, _, ttl = msgs(0)
        d = rng.choice(np.array([0, 1, 1, 1, 2, 0xFF], np.uint8), n)
        return t, s, d, ttl

    half = ids[rng.permutation(n_clients)[: n_clients // 2]]
    dup = np.concatenate([ids[:5], ids[:5], with_cat(ids[:2], CAT_GEO_CLIENT), grains[:2]])
    return [
        ("open", (np.concatenate([ids, dup]), np.arange(n_clients + len(dup), dtype=np.uint32) + 100)),
        ("deliver", msgs(1000)),
        ("close", (np.concatenate([half, half[:3], extra[:2]]), 2000, None)),
        ("deliver", msgs(2500)),
        ("ingress", ing() + (False, 5)),
        ("close", (ids[:6], 2600, rng.integers(0, 50, 6).astype(np.uint32))),
        ("drop", (2000 + 500, None)),                             # exactly at the timeout for the first close
        ("open", (np.concatenate([half[:4], extra[10:14]]), np.arange(8, dtype=np.uint32) + 900)),
        ("deliver", msgs(3000)),
        ("routes_expire", (1000 + 1900,)),                        # exactly at the expiry for the first deliver
        ("ingress", ing() + (False, 5)),
        ("ingress", ing() + (True, 5)),
        ("drop", (1 << 40, 3)),                                   # one short or more: nothing changes
        ("drop", (1 << 40, None)),
        ("routes_expire", (1 << 40,)),
    ]


LIFECYCLE_TIMEOUTS = (500, 1900)      # client_drop_timeout, route_expiry of `lifecycle`
