"""ctypes binding of libgraindispatch.so (include/graindispatch.h).

This is the Python face of the C ABI that the Orleans C# host binds with
[DllImport("graindispatch")].  It holds no routing logic:
every call goes straight through the C ABI to the gfx950 kernels.  There is
no CPU fallback -- if the shared library is missing, import fails loudly.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Iterable, List, Optional, Sequence, Tuple

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GRAINDISPATCH_LIB", os.path.join(_HERE, "libgraindispatch.so"))

# ---- constants mirrored from include/graindispatch.h --------------------------
GD_OK, GD_EINVAL, GD_ENOMEM, GD_EHIP, GD_ERCCL, GD_EFULL, GD_ESTATE, GD_ETIMEOUT = 0, -1, -2, -3, -4, -5, -6, -7
RING_DIRECTORY, RING_CONSISTENT, RING_VIRTUAL_BUCKETS = 0, 1, 2
ROUTE_OK, ROUTE_MISS, ROUTE_SYSTEM_TARGET, ROUTE_MEMBERSHIP, ROUTE_KEYEXT = 0, 1, 2, 3, 4
ROUTE_ADDRESSED, ROUTE_UNDECODED = 5, 6
FRAME_HAS_TARGET, FRAME_COMPLETE, FRAME_FALLBACK, FRAME_MALFORMED, FRAME_TARGET_KEYEXT = 1, 2, 4, 8, 16
FRAME_INVALIDATION = 32       # GD_OPT_WALK_INVALIDATION 1: the frame's CacheInvalidationHeader was stepped over
NO_ACTIVATION = 0xFFFFFFFF
NO_SILO = 0xFFFFFFFF
NO_SILO16 = 0xFFFF            # GD_NO_SILO16: the compact routes' packed GD_NO_SILO
GD_ROUTE_BAD_CLASS = 8        # gd_route_compact*: the class id is not in the class table
TTL_NONE = (1 << 63) - 1
(SEND_QUEUED, SEND_LOOPBACK, SEND_EXPIRED, SEND_NO_SILO, SEND_UNKNOWN_SILO, SEND_THROWS,
 SEND_HELD) = range(7)
PLACE_NONE, PLACE_HASH, PLACE_LOCAL, PLACE_GIVEN = range(4)
PLACED_NONE, PLACED_NEW, PLACED_JOINED, PLACED_SKIPPED = range(4)
(TURN_NONE, TURN_START, TURN_WAIT, TURN_REJECT_OVERLOADED, TURN_STUCK, TURN_FORWARD, TURN_REJECT_TRANSIENT,
 TURN_EXPIRED, TURN_RESPONSE, TURN_RESPONSE_DROPPED) = range(10)
MSG_READ_ONLY, MSG_ALWAYS_INTERLEAVE, MSG_MAY_INTERLEAVE = 1, 2, 4
CTX_VALID, CTX_NOT_READY, CTX_INVALID, CTX_STATE_MASK = 0, 1, 2, 3
CTX_HAS_RUNNING, CTX_RUNNING_READ_ONLY, CTX_REENTRANT, CTX_STATELESS_WORKER, CTX_STUCK = 4, 8, 16, 32, 64
WK_NONE, WK_IDLE, WK_NEW, WK_RANDOM, WK_HELD = range(5)
WK_NOT_GRAIN, WK_ADDED, WK_FULL = range(3)
WK_MAX_SLOT_CAPACITY = 1024
CB_NONE, CB_FIRE, CB_RESEND, CB_NO_CALLBACK, CB_GATEWAY_BACK, CB_TIMEOUT, CB_SILO_FAILED = range(7)
CB_INVALIDATE_CACHE = 1
RESP_TARGET_NOT_ME, RESP_HAS_CACHE_HEADER = 1, 2
CB_NO_SILO = 0xFFFFFFFF
ENC_OK, ENC_COPIED, ENC_SKIPPED, ENC_FALLBACK, ENC_MALFORMED, ENC_NO_ID, ENC_NO_SILO = range(7)
ENC_NO_TYPE = 0xFFFFFFFF
RSP_NONE, RSP_RESPONSE, RSP_REJECTION = range(3)
RSPST_OK, RSPST_SKIPPED, RSPST_MALFORMED, RSPST_DISCARDED, RSPST_FALLBACK = range(5)
RSP_NO_INFO = 0xFFFFFFFF
(REQ_ONE_WAY, REQ_NO_TTL, REQ_ALWAYS_INTERLEAVE, REQ_READ_ONLY, REQ_UNORDERED, REQ_IFACE_VERSION,
 REQ_TXN_REQUIRED) = (1 << k for k in range(7))
REQ_OK, REQ_UNADDRESSED, REQ_FALLBACK, REQ_NO_ID, REQ_NO_SILO = range(5)
REQ_NO_STRING = 0xFFFFFFFF
CFG_KERNEL_TIMING = 1
CFG_NO_LANE_ORDER = 2

RING_MODES = {"D": RING_DIRECTORY, "R": RING_CONSISTENT, "V": RING_VIRTUAL_BUCKETS}

# C-ABI symbols the header declares (checked by tests/test_abi.py)
EXPORTED_SYMBOLS = [
    "gd_create", "gd_destroy", "gd_last_error", "gd_abi_version", "gd_set_stream", "gd_get_stream", "gd_set_bucket_stream",
    "gd_synchronize", "gd_stats_get", "gd_host_alloc", "gd_host_free", "gd_jenkins_hash_bytes",
    "gd_jenkins_hash_u64x3", "gd_uniform_hash",
    "gd_calculate_id_hash", "gd_silo_consistent_hash", "gd_silo_uniform_hashes", "gd_silo_compare",
    "gd_ring_build", "gd_ring_set", "gd_ring_owner", "gd_ring_lookup_hashes", "gd_dir_register",
    "gd_dir_unregister", "gd_dir_lookup", "gd_dir_clear", "gd_dir_rehash", "gd_route", "gd_bucket",
    "gd_route_bucket", "gd_route_device", "gd_bucket_device", "gd_route_bucket_device",
    "gd_ring_owner_device", "gd_pack_by_shard_device", "gd_pack_routes_by_rank_device", "gd_kernel_times",
    "gd_kernel_times_reset",
    "gd_option_set", "gd_option_get", "gd_tune_reset", "gd_tune_set", "gd_tune_get", "gd_tune_agree",
    "gd_comm_info", "gd_index_stats_get", "gd_route_bound_device",
    "gd_set_kernel_timing", "gd_microbatch_create", "gd_microbatch_destroy", "gd_microbatch_keys",
    "gd_microbatch_outputs", "gd_microbatch_run", "gd_decode_frames_device", "gd_decode_frames",
    "gd_route_frames_device", "gd_route_frames", "gd_dir_split", "gd_dir_split_device",
    "gd_fanout_expand_device", "gd_fanout_route_bucket_device", "gd_fanout_route_bucket", "gd_route_nodes_device",
    "gd_pack_nodes_by_shard_device", "gd_frontier_next_device",
    "gd_cache_configure", "gd_cache_set_silos", "gd_cache_add", "gd_cache_remove", "gd_cache_lookup",
    "gd_cache_clear", "gd_cache_stats_get", "gd_cache_entries", "gd_cache_add_ext", "gd_cache_remove_ext",
    "gd_cache_lookup_ext", "gd_cache_entries_ext",
    "gd_route_frames_ext_device", "gd_route_frames_ext",
    "gd_dir_register_ext", "gd_dir_unregister_ext", "gd_dir_lookup_ext", "gd_uniform_hashes_ext",
    "gd_dir_ext_stats", "gd_route_ext", "gd_route_bucket_ext", "gd_route_ext_device", "gd_route_bucket_ext_device",
    "gd_comm_unique_id", "gd_comm_init", "gd_comm_init_local", "gd_comm_destroy", "gd_route_multi_device",
    "gd_route_multi",
    "gd_multi_fetch", "gd_route_multi_ext_device", "gd_route_multi_ext", "gd_ring_owner_ext",
    "gd_dir_split_ext", "gd_dir_upsert", "gd_dir_register_device", "gd_dir_register_device_async",
    "gd_dir_unregister_device",
    "gd_dir_set_valid_silos", "gd_dir_lookup_tagged", "gd_dir_remove_silos", "gd_activation_ids_set", "gd_dir_merge",
    "gd_actdir_add", "gd_actdir_remove", "gd_actdir_set_flags", "gd_actdir_lookup", "gd_actdir_clear",
    "gd_actdir_count", "gd_receive", "gd_receive_device", "gd_receive_frames_device", "gd_receive_frames",
    "gd_fanout_multi_device", "gd_fanout_multi", "gd_fanout_multi_fetch", "gd_dir_handoff_multi",
    "gd_fanout_multi_part_device", "gd_fanout_cascade_device",
    "gd_dir_handoff_fetch",
    "gd_send_configure", "gd_send_queues_device", "gd_send_queues", "gd_route_send_device", "gd_route_send",
    "gd_place_configure", "gd_route_place_device", "gd_route_place", "gd_route_place_bucket_device",
    "gd_route_place_bucket",
    "gd_turns_device", "gd_turns", "gd_receive_turns_device",
    "gd_decode_frames_turn_device", "gd_decode_frames_turn", "gd_receive_turns_frames_device",
    "gd_receive_turns_frames",
    "gd_turns_complete_device", "gd_turns_complete", "gd_wait_list_merge_device", "gd_wait_list_merge",
    "gd_callbacks_configure", "gd_callbacks_clear", "gd_callbacks_count", "gd_callbacks_add_device",
    "gd_callbacks_add", "gd_callbacks_set_target_device", "gd_callbacks_set_target", "gd_callbacks_lookup_device",
    "gd_callbacks_lookup", "gd_callbacks_respond_device", "gd_callbacks_respond", "gd_callbacks_expire_device",
    "gd_callbacks_expire", "gd_callbacks_break_silo_device", "gd_callbacks_break_silo",
    "gd_gateway_configure", "gd_gateway_clear", "gd_gateway_count", "gd_gateway_open_device", "gd_gateway_open",
    "gd_gateway_close_device", "gd_gateway_close", "gd_gateway_drop_device", "gd_gateway_drop",
    "gd_gateway_routes_expire_device", "gd_gateway_routes_expire", "gd_gateway_lookup_device", "gd_gateway_lookup",
    "gd_gateway_deliver_device", "gd_gateway_deliver", "gd_gateway_send_queues_device", "gd_gateway_send_queues",
    "gd_gateway_ingress_device", "gd_gateway_ingress",
    "gd_workers_configure", "gd_workers_clear", "gd_workers_count", "gd_workers_add_device", "gd_workers_add",
    "gd_workers_remove_device", "gd_workers_remove", "gd_workers_lookup_device", "gd_workers_lookup",
    "gd_workers_select_device", "gd_workers_select",
    "gd_classes_set", "gd_classes_get", "gd_route_compact", "gd_route_bucket_compact", "gd_route_compact_device",
    "gd_route_bucket_compact_device",
    "gd_encode_configure", "gd_encode_frames_device", "gd_encode_frames",
    "gd_respond_configure", "gd_respond_kinds_device", "gd_respond_kinds", "gd_silo_index_device", "gd_silo_index",
    "gd_respond_frames_device", "gd_respond_frames",
    "gd_request_configure", "gd_request_frames_device", "gd_request_frames", "gd_request_send_device",
    "gd_request_send",
    "gd_forward_kinds_device", "gd_forward_kinds", "gd_forward_frames_device", "gd_forward_frames",
    "gd_forward_send_device", "gd_forward_send",
    "gd_forward_reject_frames_device", "gd_forward_reject_frames",
    "gd_sniff_frames_device", "gd_sniff_frames", "gd_cache_invalidate_device", "gd_cache_invalidate",
    "gd_sniff_invalidate_device", "gd_sniff_invalidate",
    "gd_activate_device", "gd_activate", "gd_receive_activate_turns_device", "gd_receive_activate_turns",
    "gd_receive_activate_turns_frames_device", "gd_receive_activate_turns_frames",
    "gd_collect_configure", "gd_collect_next_ticket", "gd_collect_schedule_device", "gd_collect_schedule",
    "gd_collect_cancel_device", "gd_collect_cancel", "gd_collect_touch_device", "gd_collect_touch",
    "gd_collect_idle_device", "gd_collect_idle", "gd_collect_scan_stale_device", "gd_collect_scan_stale",
    "gd_collect_scan_all_device", "gd_collect_scan_all", "gd_collect_count_recent_device", "gd_collect_count_recent",
    "gd_cache_maintain_configure", "gd_cache_clock_set", "gd_cache_entries_age", "gd_cache_scan_device", "gd_cache_scan",
    "gd_cache_scan_fetch", "gd_dir_lookup_many_device", "gd_dir_lookup_many", "gd_cache_refresh_apply_device",
    "gd_cache_refresh_apply",
]


class gd_key(C.Structure):
    _fields_ = [("n0", C.c_uint64), ("n1", C.c_uint64), ("type_code_data", C.c_uint64)]


class gd_val(C.Structure):
    _fields_ = [("act", C.c_uint32), ("silo", C.c_uint32)]


class gd_silo_addr(C.Structure):
    _fields_ = [("ip", C.c_uint8 * 16), ("port", C.c_int32), ("generation", C.c_int32), ("is_v4", C.c_int32)]


class gd_config(C.Structure):
    _fields_ = [("struct_size", C.c_uint32), ("device", C.c_int32), ("table_capacity", C.c_uint64),
                ("my_silo", C.c_uint32), ("seed_silo", C.c_uint32), ("max_batch", C.c_uint32),
                ("flags", C.c_uint32)]


class gd_stats(C.Structure):
    _fields_ = [("routed", C.c_uint64), ("table_live", C.c_uint64), ("table_tombstones", C.c_uint64),
                ("table_capacity", C.c_uint64), ("ring_points", C.c_uint64), ("ring_mode", C.c_uint64)]


class gd_index_stats(C.Structure):
    _fields_ = [("builds", C.c_uint64), ("synced_slots", C.c_uint64), ("last_build_ms", C.c_double),
                ("current", C.c_uint32), ("types8", C.c_uint32), ("act_bits8", C.c_uint32),
                ("silo_bits8", C.c_uint32), ("n0_live", C.c_uint32), ("out8", C.c_uint32)]


class gd_cache_stats(C.Structure):
    _fields_ = [("count", C.c_uint64), ("accesses", C.c_uint64), ("hits", C.c_uint64),
                ("next_generation", C.c_uint64), ("max_size", C.c_uint64), ("capacity", C.c_uint64)]


class gd_kernel_time(C.Structure):
    _fields_ = [("name", C.c_char * 48), ("launches", C.c_uint64), ("total_ms", C.c_double)]


class gd_frame_fields(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in
                ("flags", "target_grain", "mask", "target_activation", "sending_activation", "sending_grain",
                 "target_silo", "sending_silo", "correlation_id", "category", "direction")]


# gd_frame_fields member -> (numpy dtype, trailing shape) of the host arrays
FRAME_FIELDS = {"flags": (np.uint32, ()), "target_grain": (np.uint64, (3,)), "mask": (np.uint32, ()),
                "target_activation": (np.uint64, (3,)), "sending_activation": (np.uint64, (3,)),
                "sending_grain": (np.uint64, (3,)), "target_silo": (np.uint8, (24,)),
                "sending_silo": (np.uint8, (24,)), "correlation_id": (np.int64, ()),
                "category": (np.uint8, ()), "direction": (np.uint8, ())}


class gd_frame_turn_fields(C.Structure):
    _fields_ = [(name, C.c_void_p) for name in
                ("ttl", "forward_count", "msg_flags", "result", "rejection_type", "resend_count")]


# gd_frame_turn_fields member -> numpy dtype of the host arrays
FRAME_TURN_FIELDS = {"ttl": np.int64, "forward_count": np.uint8, "msg_flags": np.uint8, "result": np.uint8,
                     "rejection_type": np.uint8, "resend_count": np.int32}


class gd_multi_result(C.Structure):
    _fields_ = [("n_recv", C.c_uint32), ("n_act", C.c_uint32)] + [
        (f, C.c_void_p) for f in ("recv_keys", "recv_idx", "recv_src", "silo", "act", "status", "perm", "offsets",
                                  "ret_silo", "ret_act", "ret_status")]


class gd_fanout_hop(C.Structure):
    _fields_ = [("n_frontier", C.c_uint32), ("frontier", C.c_void_p), ("n_sent", C.c_uint64), ("n_recv", C.c_uint32)] + [
        (f, C.c_void_p) for f in ("target", "sender", "src", "silo", "act", "status", "perm", "offsets")]


class gd_handoff_result(C.Structure):
    _fields_ = [("n_sent", C.c_uint64), ("n_recv", C.c_uint32)] + [
        (f, C.c_void_p) for f in ("recv_keys", "recv_ids", "recv_act", "recv_silo", "recv_src", "status", "dropped")]


GD_HANDOFF_ADD, GD_HANDOFF_REMOVE = 0, 1
GD_MERGE_TAG_MULTI_INSTANCE = 0x80000000
GD_MERGE_INSERTED, GD_MERGE_KEPT, GD_MERGE_SAME, GD_MERGE_DROPPED, GD_MERGE_HOST, GD_MERGE_UNION = 0, 1, 2, 3, 4, 5
ACTDIR_VALID, ACTDIR_SYSTEM_TARGET, ACTDIR_STATELESS_WORKER = 1, 2, 4
(RECV_ACTIVATION, RECV_SYSTEM_TARGET, RECV_NULL_CONTEXT, RECV_REJECT_UNKNOWN, RECV_REJECT_OVERLOADED, RECV_DROPPED,
 RECV_UNDECODED) = range(7)


class gd_recv_limits(C.Structure):
    _fields_ = [("request_count", C.c_void_p), ("hard_limit", C.c_int32), ("hard_limit_stateless_worker", C.c_int32)]


class gd_turn_state(C.Structure):
    _fields_ = [("ctx_flags", C.c_void_p), ("num_running", C.c_void_p), ("request_count", C.c_void_p),
                ("hard_limit", C.c_int32), ("hard_limit_stateless_worker", C.c_int32),
                ("max_forward_count", C.c_uint32), ("allow_call_chain_reentrancy", C.c_int32)]


class gd_wait_list(C.Structure):
    _fields_ = [("offsets", C.c_void_p), ("msg", C.c_void_p), ("flags", C.c_void_p)]


class gd_collect_state(C.Structure):
    _fields_ = [("ticket", C.c_void_p), ("became_idle", C.c_void_p), ("keep_alive_until", C.c_void_p),
                ("age_limit", C.c_void_p), ("flags", C.c_void_p)]


MSG_CALL_CHAIN = 8
DONE_IS_RUNNING, DONE_PUMP_ONLY = 1, 2
PUMP_BECAME_IDLE, PUMP_RUNNING_CLEARED, PUMP_RUNNING_SET = 1, 2, 4
# activation collector (gd_collect_*): flag bits; schedule statuses; touch / idle answers; scan verdicts
GD_COL_EXEMPT, GD_COL_CANCELLED = 1, 2
(GD_COL_SCHEDULED, GD_COL_OUT_OF_RANGE, GD_COL_SKIPPED_EXEMPT, GD_COL_SKIPPED_NO_LIMIT, GD_COL_THROWS_TIMEOUT,
 GD_COL_THROWS_EARLY, GD_COL_THROWS_TICKETED) = range(7)
GD_COL_FALSE, GD_COL_TRUE, GD_COL_THROWS, GD_COL_NO_PART = range(4)
GD_COL_BAD_STATE, GD_COL_KEPT_ALIVE, GD_COL_ACTIVE, GD_COL_NOT_STALE, GD_COL_COLLECT = range(1, 6)
GD_COL_NOT_ADDED = 0x80

GD_COMM_ID_BYTES = 128
GD_ACT_MULTI = 0xFFFFFFFE
GD_ROUTE_MULTI_ACT = 7
GD_KEYEXT_NULL = -1
GD_KEYEXT_HOST = -2


class gd_cache_scan_result(C.Structure):
    _fields_ = [("counts", C.c_uint64 * 5), ("n_owners", C.c_uint32), ("n", C.c_uint32), ("ext_bytes_len", C.c_uint64),
                ("owner", C.c_void_p), ("offsets", C.c_void_p), ("keys", C.c_void_p), ("etags", C.c_void_p),
                ("slots", C.c_void_p), ("ext_len", C.c_void_p), ("ext_off", C.c_void_p), ("ext_bytes", C.c_void_p)]


GD_CM_SEEN, GD_CM_SELF_OWNED, GD_CM_FRESH, GD_CM_DROPPED, GD_CM_REFRESH = range(5)
GD_LM_SAME, GD_LM_ABSENT, GD_LM_UPDATED, GD_LM_HOST = range(4)
GD_CR_UPDATED, GD_CR_REMOVED, GD_CR_NOT_PRESENT, GD_CR_FRESHENED, GD_CR_SKIPPED, GD_CR_DEFERRED = range(6)


class gd_key_ext(C.Structure):
    _fields_ = [("bytes", C.c_void_p), ("offset", C.c_void_p), ("length", C.c_void_p), ("bytes_len", C.c_uint64)]


class KeyExtBatch:
    """A batch's KeyExt strings in the gd_key_ext layout.  Items: bytes (UTF-8), str (encoded
    UTF-8), None (KeyExt null) or GD_KEYEXT_HOST (leave to the C# path).  Holds the arrays the
    struct points at."""

    def __init__(self, exts):
        n = len(exts)
        self.offset = np.zeros(n, np.uint64)
        self.length = np.zeros(n, np.int32)
        parts, pos = [], 0
        for i, e in enumerate(exts):
            if e is None:
                self.length[i] = GD_KEYEXT_NULL
            elif isinstance(e, (int, np.integer)):
                self.length[i] = int(e)
            else:
                b = e.encode("utf-8") if isinstance(e, str) else bytes(e)
                self.offset[i] = pos
                self.length[i] = len(b)
                parts.append(b)
                pos += len(b)
        self.blob = np.frombuffer(b"".join(parts) + b"\0", dtype=np.uint8).copy()
        self.struct = gd_key_ext(self.blob.ctypes.data, self.offset.ctypes.data, self.length.ctypes.data, pos)


class gd_request_batch(C.Structure):
    _fields_ = [("target", C.c_void_p), ("target_ext", C.POINTER(gd_key_ext)), ("sender_grain", C.c_void_p),
                ("sender_ext", C.POINTER(gd_key_ext)), ("sender_act", C.c_void_p), ("options", C.c_void_p),
                ("generic", C.c_void_p), ("debug", C.c_void_p), ("id_base", C.c_int64), ("ttl_ticks", C.c_int64),
                ("body", C.c_void_p), ("body_off", C.c_void_p)]


class gd_forward_batch(C.Structure):
    _fields_ = [("buf", C.c_void_p), ("buf_len", C.c_uint64), ("frame_off", C.c_void_p), ("kind", C.c_void_p),
                ("old_act", C.c_void_p), ("fwd_silo", C.c_void_p), ("fwd_act", C.c_void_p),
                ("max_forward_count", C.c_int32), ("local_silo", C.c_uint32)]


GD_FWD_NONE, GD_FWD_FORWARD = 0, 1
(GD_FWDST_OK_ADDRESSED, GD_FWDST_OK_UNADDRESSED, GD_FWDST_SKIPPED, GD_FWDST_MALFORMED, GD_FWDST_FALLBACK,
 GD_FWDST_REJECT, GD_FWDST_NO_SILO, GD_FWDST_NO_ID) = range(8)
(GD_FWDREJ_OK, GD_FWDREJ_SKIPPED, GD_FWDREJ_MALFORMED, GD_FWDREJ_FALLBACK, GD_FWDREJ_MAY_FORWARD,
 GD_FWDREJ_DISCARDED, GD_FWDREJ_NO_SILO, GD_FWDREJ_NO_ID) = range(8)



class gd_sniff_out(C.Structure):
    _fields_ = [("count", C.c_void_p), ("ent_off", C.c_void_p), ("status", C.c_void_p), ("flags", C.c_void_p),
                ("ent_frame", C.c_void_p), ("ent_silo", C.c_void_p), ("ent_grain", C.c_void_p),
                ("ent_ext_off", C.c_void_p), ("ent_ext_len", C.c_void_p), ("ent_act_id", C.c_void_p)]


SNIFF_FIELDS = tuple(f for f, _ in gd_sniff_out._fields_)
GD_SNIFF_NONE, GD_SNIFF_OK, GD_SNIFF_MALFORMED = range(3)
GD_SNIFF_FLAG_RETURNED, GD_SNIFF_FLAG_UNKNOWN = 1, 2
GD_INV_MISS, GD_INV_REMOVED, GD_INV_KEPT, GD_INV_HOST, GD_INV_NO_ID = range(5)


class gd_activate_io(C.Structure):
    _fields_ = [("new_placement", C.c_void_p), ("terminating", C.c_int32), ("ctx_base", C.c_uint32),
                ("new_ctx", C.c_void_p), ("cap_new", C.c_uint32), ("kind", C.c_void_p), ("new_idx", C.c_void_p),
                ("n_new", C.c_void_p), ("gone_idx", C.c_void_p), ("n_gone", C.c_void_p), ("n_proposed", C.c_void_p)]


(GD_ACTV_NONE, GD_ACTV_FOUND, GD_ACTV_CREATED, GD_ACTV_EXPIRED, GD_ACTV_HOST, GD_ACTV_NONEXISTENT,
 GD_ACTV_NONEXISTENT_RESPONSE) = range(7)

GD_MULTI_RETURN_ROUTES = 1
GD_MULTI_KEYS_READY = 2
GD_MULTI_FORWARD = 4
GD_MULTI_NO_KEYS = 8


class ScanLists(dict):
    """cache_scan's request lists: owner silo -> (keys, etags, exts) in list order; .owners, .offsets, .slots the CSR."""


class GrainDispatchError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"graindispatch error {code}: {msg}")
        self.code = code


def _load() -> C.CDLL:
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"libgraindispatch.so not built at {LIB_PATH}; run __graft_entry__.build()")
    # One HIP runtime per process.  torch ships its own libamdhip64 / libhsa-runtime64 with the
    # same sonames as /opt/rocm's but is linked against the unversioned names: if this library
    # loaded /opt/rocm's copies first, a later `import torch` would load its copies beside them
    # and whichever HSA runtime initialises second finds no device.  With torch imported first,
    # our NEEDED libamdhip64.so.7 resolves to the copy torch already holds.
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(LIB_PATH)
    P, U32, U64, I32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32
    I64, CS = C.c_int64, C.POINTER(gd_collect_state)
    sig = {
        "gd_create": (C.c_int, [C.POINTER(gd_config), C.POINTER(P)]),
        "gd_destroy": (None, [P]),
        "gd_last_error": (C.c_char_p, [P]),
        "gd_abi_version": (C.c_int, []),
        "gd_set_stream": (C.c_int, [P, P]),
        "gd_set_bucket_stream": (C.c_int, [P, P]),
        "gd_get_stream": (P, [P]),
        "gd_host_alloc": (C.c_int, [C.c_size_t, P]),
        "gd_host_free": (C.c_int, [P]),
        "gd_synchronize": (C.c_int, [P]),
        "gd_stats_get": (C.c_int, [P, C.POINTER(gd_stats)]),
        "gd_index_stats_get": (C.c_int, [P, C.POINTER(gd_index_stats)]),
        "gd_jenkins_hash_bytes": (U32, [P, C.c_size_t]),
        "gd_jenkins_hash_u64x3": (U32, [U64, U64, U64]),
        "gd_uniform_hash": (U32, [C.POINTER(gd_key)]),
        "gd_calculate_id_hash": (I32, [C.c_char_p]),
        "gd_silo_consistent_hash": (I32, [C.POINTER(gd_silo_addr)]),
        "gd_silo_uniform_hashes": (C.c_int, [C.POINTER(gd_silo_addr), U32, P]),
        "gd_silo_compare": (C.c_int, [C.POINTER(gd_silo_addr), C.POINTER(gd_silo_addr)]),
        "gd_ring_build": (C.c_int, [C.c_int, P, U32, U32, P, P, C.POINTER(U32)]),
        "gd_ring_set": (C.c_int, [P, C.c_int, P, P, U32]),
        "gd_ring_owner": (C.c_int, [P, P, U32, P]),
        "gd_ring_lookup_hashes": (C.c_int, [P, P, U32, P]),
        "gd_dir_register": (C.c_int, [P, P, P, U32, P, P]),
        "gd_dir_unregister": (C.c_int, [P, P, P, U32, P]),
        "gd_dir_register_device": (C.c_int, [P, P, P, U32, P, P]),
        "gd_dir_register_device_async": (C.c_int, [P, P, P, U32, P, P]),
        "gd_dir_unregister_device": (C.c_int, [P, P, P, U32, P]),
        "gd_dir_set_valid_silos": (C.c_int, [P, P, U32]),
        "gd_dir_lookup_tagged": (C.c_int, [P, P, U32, P, P, P]),
        "gd_cache_maintain_configure": (C.c_int, [P, C.c_int64, C.c_int64, C.c_double, C.c_int64]),
        "gd_cache_clock_set": (C.c_int, [P, C.c_int64]),
        "gd_cache_entries_age": (C.c_int, [P, P, P, P, U64, C.POINTER(U64)]),
        "gd_cache_scan_device": (C.c_int, [P, C.c_int64, C.POINTER(gd_cache_scan_result)]),
        "gd_cache_scan": (C.c_int, [P, C.c_int64, P, C.POINTER(U32), C.POINTER(U32), C.POINTER(U64)]),
        "gd_cache_scan_fetch": (C.c_int, [P, P, P, P, P, P, P, P, P, U32, U32, U64]),
        "gd_dir_lookup_many_device": (C.c_int, [P, P, P, U32, P, P, P]),
        "gd_dir_lookup_many": (C.c_int, [P, P, P, U32, P, P, P]),
        "gd_cache_refresh_apply_device": (C.c_int, [P, C.c_int64, P, C.POINTER(gd_key_ext), P, U32, P]),
        "gd_cache_refresh_apply": (C.c_int, [P, C.c_int64, P, C.POINTER(gd_key_ext), P, P, P, U32, P]),
        "gd_dir_remove_silos": (C.c_int, [P, P, U32, C.POINTER(U64), C.POINTER(U64), C.POINTER(U64)]),
        "gd_activation_ids_set": (C.c_int, [P, P, P, U32]),
        "gd_dir_merge": (C.c_int, [P, P, P, P, U32, P, P]),
        "gd_actdir_add": (C.c_int, [P, P, P, P, U32, P]),
        "gd_actdir_remove": (C.c_int, [P, P, U32, P]),
        "gd_actdir_set_flags": (C.c_int, [P, P, P, U32, P]),
        "gd_actdir_lookup": (C.c_int, [P, P, U32, P, P, P]),
        "gd_actdir_clear": (C.c_int, [P]),
        "gd_actdir_count": (C.c_int, [P, C.POINTER(U64)]),
        "gd_receive": (C.c_int, [P, P, P, P, U32, U32, C.POINTER(gd_recv_limits), P, P, P, P]),
        "gd_receive_device": (C.c_int, [P, P, P, P, U32, U32, C.POINTER(gd_recv_limits), P, P, P, P]),
        "gd_receive_frames_device": (C.c_int, [P, P, U64, P, U32, U32, C.POINTER(gd_recv_limits),
                                               C.POINTER(gd_frame_fields), P, P, P, P]),
        "gd_receive_frames": (C.c_int, [P, P, U64, P, U32, U32, C.POINTER(gd_recv_limits), C.POINTER(gd_frame_fields),
                                        P, P, P, P]),
        "gd_send_configure": (C.c_int, [P, P, U32, U32]),
        "gd_send_queues_device": (C.c_int, [P, P, P, P, P, U32, P, P, P, P]),
        "gd_send_queues": (C.c_int, [P, P, P, P, P, U32, P, P, P, P]),
        "gd_route_send_device": (C.c_int, [P, P, U32, P, P, P, P, P, P, P, P, P]),
        "gd_route_send": (C.c_int, [P, P, U32, P, P, P, P, P, P, P, P, P]),
        "gd_place_configure": (C.c_int, [P, P, U32, P, C.c_int]),
        "gd_route_place_device": (C.c_int, [P, P, U32, P, C.c_int, P, U32, P, P, P, P, P, C.POINTER(U32),
                                            C.POINTER(U32)]),
        "gd_route_place": (C.c_int, [P, P, U32, P, C.c_int, P, U32, P, P, P, P, P, C.POINTER(U32), C.POINTER(U32)]),
        "gd_route_place_bucket_device": (C.c_int, [P, P, U32, P, C.c_int, P, U32, P, P, P, P, P, C.POINTER(U32),
                                                   C.POINTER(U32), U32, P, P]),
        "gd_route_place_bucket": (C.c_int, [P, P, U32, P, C.c_int, P, U32, P, P, P, P, P, C.POINTER(U32),
                                            C.POINTER(U32), U32, P, P]),
        "gd_turns_device": (C.c_int, [P] + [P] * 8 + [U32, U32, C.POINTER(gd_turn_state)] + [P] * 7),
        "gd_turns": (C.c_int, [P] + [P] * 8 + [U32, U32, C.POINTER(gd_turn_state)] + [P] * 7),
        "gd_receive_turns_device": (C.c_int, [P, P, P, P, U32, U32, C.POINTER(gd_recv_limits), P, P, P, P, P, P, P, P,
                                              C.POINTER(gd_turn_state)] + [P] * 7),
        "gd_decode_frames_turn_device": (C.c_int, [P, P, U64, P, U32, C.POINTER(gd_frame_fields),
                                                   C.POINTER(gd_frame_turn_fields)]),
        "gd_decode_frames_turn": (C.c_int, [P, P, U64, P, U32, C.POINTER(gd_frame_fields),
                                            C.POINTER(gd_frame_turn_fields)]),
        "gd_receive_turns_frames_device": (C.c_int, [P, P, U64, P, U32, U32, C.POINTER(gd_recv_limits),
                                                     C.POINTER(gd_frame_fields), C.POINTER(gd_frame_turn_fields),
                                                     P, P, P, P, C.c_int64, P, C.POINTER(gd_turn_state)] + [P] * 7),
        "gd_receive_turns_frames": (C.c_int, [P, P, U64, P, U32, U32, C.POINTER(gd_recv_limits),
                                              C.POINTER(gd_frame_fields), C.POINTER(gd_frame_turn_fields),
                                              P, P, P, P, C.c_int64, P, C.POINTER(gd_turn_state)] + [P] * 7),
        "gd_turns_complete_device": (C.c_int, [P, P, P, U32, U32, P, P, C.POINTER(gd_wait_list), U32] + [P] * 8),
        "gd_turns_complete": (C.c_int, [P, P, P, U32, U32, P, P, C.POINTER(gd_wait_list), U32] + [P] * 8),
        "gd_wait_list_merge_device": (C.c_int, [P, C.POINTER(gd_wait_list), P, U32, P, P, U32, P, U32, P, P, P, C.c_int,
                                                U32, P, P, P, P]),
        "gd_wait_list_merge": (C.c_int, [P, C.POINTER(gd_wait_list), P, U32, P, P, U32, P, U32, P, P, P, C.c_int, U32,
                                         P, P, P, P]),
        "gd_callbacks_configure": (C.c_int, [P, U64, U32, C.c_int, C.c_int64]),
        "gd_callbacks_clear": (C.c_int, [P]),
        "gd_callbacks_count": (C.c_int, [P, C.POINTER(U64), C.POINTER(U64)]),
        "gd_callbacks_add_device": (C.c_int, [P, P, P, P, U32, P]),
        "gd_callbacks_add": (C.c_int, [P, P, P, P, U32, P]),
        "gd_callbacks_set_target_device": (C.c_int, [P, P, P, U32, P]),
        "gd_callbacks_set_target": (C.c_int, [P, P, P, U32, P]),
        "gd_callbacks_lookup_device": (C.c_int, [P, P, U32, P, P, P, P]),
        "gd_callbacks_lookup": (C.c_int, [P, P, U32, P, P, P, P]),
        "gd_callbacks_respond_device": (C.c_int, [P, P, P, P, P, P, U32, P, P, P, P, P]),
        "gd_callbacks_respond": (C.c_int, [P, P, P, P, P, P, U32, P, P, P, P, P]),
        "gd_callbacks_expire_device": (C.c_int, [P, C.c_int64, U32, P, P, P, P]),
        "gd_callbacks_expire": (C.c_int, [P, C.c_int64, U32, P, P, P, P]),
        "gd_callbacks_break_silo_device": (C.c_int, [P, U32, U32, P, P, P, P]),
        "gd_callbacks_break_silo": (C.c_int, [P, U32, U32, P, P, P, P]),
        "gd_gateway_configure": (C.c_int, [P, U32, C.c_int64, C.c_int64, U64]),
        "gd_gateway_clear": (C.c_int, [P]),
        "gd_gateway_count": (C.c_int, [P] + [C.POINTER(U64)] * 4),
        "gd_gateway_open_device": (C.c_int, [P, P, P, U32, P, P, P, P]),
        "gd_gateway_open": (C.c_int, [P, P, P, U32, P, P, P, P]),
        "gd_gateway_close_device": (C.c_int, [P, P, P, U32, C.c_int64, P]),
        "gd_gateway_close": (C.c_int, [P, P, P, U32, C.c_int64, P]),
        "gd_gateway_drop_device": (C.c_int, [P, C.c_int64, U32, P, P, P, P]),
        "gd_gateway_drop": (C.c_int, [P, C.c_int64, U32, P, P, P, P]),
        "gd_gateway_routes_expire_device": (C.c_int, [P, C.c_int64, P]),
        "gd_gateway_routes_expire": (C.c_int, [P, C.c_int64, P]),
        "gd_gateway_lookup_device": (C.c_int, [P, P, U32] + [P] * 9),
        "gd_gateway_lookup": (C.c_int, [P, P, U32] + [P] * 9),
        "gd_gateway_deliver_device": (C.c_int, [P, P, P, P, P, U32, C.c_int64, P, P, P, P, P]),
        "gd_gateway_deliver": (C.c_int, [P, P, P, P, P, U32, C.c_int64, P, P, P, P, P]),
        "gd_gateway_send_queues_device": (C.c_int, [P] + [P] * 7 + [U32, C.c_int64] + [P] * 5),
        "gd_gateway_send_queues": (C.c_int, [P] + [P] * 7 + [U32, C.c_int64] + [P] * 5),
        "gd_gateway_ingress_device": (C.c_int, [P, P, P, P, P, U32, C.c_int, P, P, P, P, P]),
        "gd_gateway_ingress": (C.c_int, [P, P, P, P, P, U32, C.c_int, P, P, P, P, P]),
        "gd_workers_configure": (C.c_int, [P, U64, U32, U32]),
        "gd_workers_clear": (C.c_int, [P]),
        "gd_workers_count": (C.c_int, [P] + [C.POINTER(U64)] * 2),
        "gd_workers_add_device": (C.c_int, [P, P, P, P, U32, P]),
        "gd_workers_add": (C.c_int, [P, P, P, P, U32, P]),
        "gd_workers_remove_device": (C.c_int, [P, P, P, U32, P]),
        "gd_workers_remove": (C.c_int, [P, P, P, U32, P]),
        "gd_workers_lookup_device": (C.c_int, [P, P, U32, P, P, P]),
        "gd_workers_lookup": (C.c_int, [P, P, U32, P, P, P]),
        "gd_workers_select_device": (C.c_int, [P, P, U32, P, P, U32, U32] + [P] * 7),
        "gd_workers_select": (C.c_int, [P, P, U32, P, P, U32, U32] + [P] * 7),
        "gd_classes_set": (C.c_int, [P, P, U32]),
        "gd_classes_get": (C.c_int, [P, P, U32, C.POINTER(U32)]),
        "gd_route_compact": (C.c_int, [P, P, P, U32, U32, P, P, P]),
        "gd_route_bucket_compact": (C.c_int, [P, P, P, U32, U32, U32, P, P, P, P, P]),
        "gd_route_compact_device": (C.c_int, [P, P, P, U32, U32, P, P, P, P]),
        "gd_route_bucket_compact_device": (C.c_int, [P, P, P, U32, U32, U32, P, P, P, P, P, P]),
        "gd_encode_configure": (C.c_int, [P, P, U32, P, P, U32]),
        "gd_encode_frames_device": (C.c_int, [P, P, U64, P, U32, P, P, P, P, P, P, P, U64, P, P]),
        "gd_encode_frames": (C.c_int, [P, P, U64, P, U32, P, P, P, P, P, P, P, U64, P, P, C.POINTER(U64)]),
        "gd_respond_configure": (C.c_int, [P, P, P, U32]),
        "gd_respond_kinds_device": (C.c_int, [P, P, P, U32, P, P]),
        "gd_respond_kinds": (C.c_int, [P, P, P, U32, P, P]),
        "gd_silo_index_device": (C.c_int, [P, P, U32, P]),
        "gd_silo_index": (C.c_int, [P, P, U32, P]),
        "gd_respond_frames_device": (C.c_int, [P, P, U64, P, U32, P, P, P, P, P, P, P, P, U64, P, P]),
        "gd_respond_frames": (C.c_int, [P, P, U64, P, U32, P, P, P, P, P, P, P, P, U64, P, P, C.POINTER(U64)]),
        "gd_request_configure": (C.c_int, [P, P, P, U32]),
        "gd_request_frames_device": (C.c_int, [P, C.POINTER(gd_request_batch), U32, P, P, P, P, P, P, P, U64, P, P]),
        "gd_request_frames": (C.c_int, [P, C.POINTER(gd_request_batch), U32, P, P, P, P, P, P, P, U64, P, P,
                                        C.POINTER(U64)]),
        "gd_forward_kinds_device": (C.c_int, [P, P, U32, P]),
        "gd_forward_kinds": (C.c_int, [P, P, U32, P]),
        "gd_forward_frames_device": (C.c_int, [P, C.POINTER(gd_forward_batch), U32, P, P, P, P, P, P, P, U64, P, P, P]),
        "gd_forward_frames": (C.c_int, [P, C.POINTER(gd_forward_batch), U32, P, P, P, P, P, P, P, U64, P, P, P,
                                        C.POINTER(U64)]),
        "gd_forward_reject_frames_device": (C.c_int, [P, C.POINTER(gd_forward_batch), U32, P, P, P, P, P, U64, P, P]),
        "gd_forward_reject_frames": (C.c_int, [P, C.POINTER(gd_forward_batch), U32, P, P, P, P, P, U64, P, P,
                                               C.POINTER(U64)]),
        "gd_sniff_frames_device": (C.c_int, [P, P, U64, P, U32, C.POINTER(gd_sniff_out), U32]),
        "gd_sniff_frames": (C.c_int, [P, P, U64, P, U32, C.POINTER(gd_sniff_out), U32, C.POINTER(U32)]),
        "gd_cache_invalidate_device": (C.c_int, [P, P, C.POINTER(gd_key_ext), P, U32, P, P]),
        "gd_cache_invalidate": (C.c_int, [P, P, C.POINTER(gd_key_ext), P, U32, P]),
        "gd_sniff_invalidate_device": (C.c_int, [P, P, U64, P, U32, C.POINTER(gd_sniff_out), U32, P]),
        "gd_sniff_invalidate": (C.c_int, [P, P, U64, P, U32, C.POINTER(gd_sniff_out), U32, P, C.POINTER(U32)]),
        "gd_activate_device": (C.c_int, [P] + [P] * 7 + [U32, U32, C.c_int, U32, P, U32] + [P] * 8),
        "gd_activate": (C.c_int, [P] + [P] * 7 + [U32, U32, C.c_int, U32, P, U32] + [P] * 8),
        "gd_receive_activate_turns_device": (C.c_int, [P, P, P, P, U32, U32, C.POINTER(gd_recv_limits), P, P, P, P, P,
                                                       P, P, P, C.POINTER(gd_turn_state)] + [P] * 7 +
                                             [C.POINTER(gd_activate_io)]),
        "gd_receive_activate_turns": (C.c_int, [P, P, P, P, U32, U32, C.POINTER(gd_recv_limits), P, P, P, P, P, P, P, P,
                                                C.POINTER(gd_turn_state)] + [P] * 7 + [C.POINTER(gd_activate_io)]),
        "gd_receive_activate_turns_frames_device": (C.c_int, [P, P, U64, P, U32, U32, C.POINTER(gd_recv_limits),
                                                              C.POINTER(gd_frame_fields),
                                                              C.POINTER(gd_frame_turn_fields), P, P, P, P, C.c_int64, P,
                                                              C.POINTER(gd_turn_state)] + [P] * 7 +
                                                    [C.POINTER(gd_activate_io)]),
        "gd_receive_activate_turns_frames": (C.c_int, [P, P, U64, P, U32, U32, C.POINTER(gd_recv_limits),
                                                       C.POINTER(gd_frame_fields), C.POINTER(gd_frame_turn_fields),
                                                       P, P, P, P, C.c_int64, P, C.POINTER(gd_turn_state)] + [P] * 7 +
                                             [C.POINTER(gd_activate_io)]),
        "gd_forward_send_device": (C.c_int, [P, C.POINTER(gd_forward_batch), U32, P, P, P, P, P, P, P, P, U64, P, P,
                                             P]),
        "gd_forward_send": (C.c_int, [P, C.POINTER(gd_forward_batch), U32, P, P, P, P, P, P, P, P, U64, P, P, P,
                                      C.POINTER(U64)]),
        "gd_request_send_device": (C.c_int, [P, C.POINTER(gd_request_batch), U32, P, P, P, P, P, P, P, P, U64, P, P]),
        "gd_request_send": (C.c_int, [P, C.POINTER(gd_request_batch), U32, P, P, P, P, P, P, P, P, U64, P, P,
                                      C.POINTER(U64)]),
        "gd_collect_configure": (C.c_int, [P, I64, I64]),
        "gd_collect_next_ticket": (C.c_int, [P, C.POINTER(I64)]),
        "gd_collect_schedule_device": (C.c_int, [P, CS, U32, P, U32, I64, P]),
        "gd_collect_schedule": (C.c_int, [P, CS, U32, P, U32, I64, P]),
        "gd_collect_cancel_device": (C.c_int, [P, CS, U32, P, U32, P]),
        "gd_collect_cancel": (C.c_int, [P, CS, U32, P, U32, P]),
        "gd_collect_touch_device": (C.c_int, [P, CS, U32, P, P, P, U32, I64, P]),
        "gd_collect_touch": (C.c_int, [P, CS, U32, P, P, P, U32, I64, P]),
        "gd_collect_idle_device": (C.c_int, [P, CS, U32, P, I64, P]),
        "gd_collect_idle": (C.c_int, [P, CS, U32, P, I64, P]),
        "gd_collect_scan_stale_device": (C.c_int, [P, CS, U32, P, P, P, I64, P, P, P]),
        "gd_collect_scan_stale": (C.c_int, [P, CS, U32, P, P, P, I64, P, P, P]),
        "gd_collect_scan_all_device": (C.c_int, [P, CS, U32, P, P, P, I64, I64, P, P, P]),
        "gd_collect_scan_all": (C.c_int, [P, CS, U32, P, P, P, I64, I64, P, P, P]),
        "gd_collect_count_recent_device": (C.c_int, [P, CS, U32, I64, I64, I64, P]),
        "gd_collect_count_recent": (C.c_int, [P, CS, U32, I64, I64, I64, P]),
        "gd_dir_upsert": (C.c_int, [P, P, P, U32, P]),
        "gd_dir_lookup": (C.c_int, [P, P, U32, P, P]),
        "gd_dir_clear": (C.c_int, [P]),
        "gd_dir_rehash": (C.c_int, [P, U64]),
        "gd_route": (C.c_int, [P, P, U32, P, P, P]),
        "gd_bucket": (C.c_int, [P, P, U32, U32, P, P]),
        "gd_route_bucket": (C.c_int, [P, P, U32, U32, P, P, P, P, P]),
        "gd_route_device": (C.c_int, [P, P, U32, P, P, P]),
        "gd_route_bound_device": (C.c_int, [P, P, U32, P, P, P]),
        "gd_bucket_device": (C.c_int, [P, P, U32, U32, P, P]),
        "gd_route_bucket_device": (C.c_int, [P, P, U32, U32, P, P, P, P, P]),
        "gd_ring_owner_device": (C.c_int, [P, P, U32, P]),
        "gd_pack_by_shard_device": (C.c_int, [P, P, U32, U32, P, P, P]),
        "gd_pack_routes_by_rank_device": (C.c_int, [P, P, P, P, U32, U32, U32, P, P, P]),
        "gd_kernel_times": (C.c_int, [P, C.POINTER(gd_kernel_time), U32, C.POINTER(U32)]),
        "gd_kernel_times_reset": (C.c_int, [P]),
        "gd_set_kernel_timing": (C.c_int, [P, C.c_int]),
        "gd_microbatch_create": (C.c_int, [P, U32, U32, C.POINTER(P)]),
        "gd_microbatch_destroy": (None, [P]),
        "gd_microbatch_keys": (P, [P]),
        "gd_microbatch_outputs": (C.c_int, [P] + [C.POINTER(P)] * 7),
        "gd_microbatch_run": (C.c_int, [P, U32, C.c_int]),
        "gd_decode_frames_device": (C.c_int, [P, P, U64, P, U32, C.POINTER(gd_frame_fields)]),
        "gd_decode_frames": (C.c_int, [P, P, U64, P, U32, C.POINTER(gd_frame_fields)]),
        "gd_route_frames_device": (C.c_int, [P, P, U64, P, U32, U32, C.POINTER(gd_frame_fields), P, P, P, P, P]),
        "gd_route_frames": (C.c_int, [P, P, U64, P, U32, U32, C.POINTER(gd_frame_fields), P, P, P, P, P]),
        "gd_route_frames_ext_device": (C.c_int, [P, P, U64, P, U32, U32, C.POINTER(gd_frame_fields), P, P, P, P, P]),
        "gd_route_frames_ext": (C.c_int, [P, P, U64, P, U32, U32, C.POINTER(gd_frame_fields), P, P, P, P, P]),
        "gd_dir_split": (C.c_int, [P, P, U32, C.c_int, P, P, U64, C.POINTER(U64)]),
        "gd_dir_split_device": (C.c_int, [P, P, U32, C.c_int, P, P, U64, C.POINTER(U64)]),
        "gd_fanout_expand_device": (C.c_int, [P, P, P, U32, P, U32, P, P, U64, C.POINTER(U64)]),
        "gd_fanout_route_bucket_device": (C.c_int, [P, P, P, U32, P, U32, I32, U32] + [P] * 7 + [U64, C.POINTER(U64)]),
        "gd_fanout_route_bucket": (C.c_int, [P, P, P, U32, P, U32, I32, U32] + [P] * 7 + [U64, C.POINTER(U64)]),
        "gd_route_nodes_device": (C.c_int, [P, P, U32, I32, P, P, P]),
        "gd_pack_nodes_by_shard_device": (C.c_int, [P, P, P, U32, I32, U32, P, P, P]),
        "gd_frontier_next_device": (C.c_int, [P, P, U32, P, P, C.POINTER(U32)]),
        "gd_cache_configure": (C.c_int, [P, U32, P, P, U32]),
        "gd_cache_set_silos": (C.c_int, [P, P, P, U32]),
        "gd_cache_add": (C.c_int, [P, P, P, P, U32]),
        "gd_cache_remove": (C.c_int, [P, P, U32, P]),
        "gd_cache_lookup": (C.c_int, [P, P, U32, P, P, P]),
        "gd_cache_clear": (C.c_int, [P]),
        "gd_cache_stats_get": (C.c_int, [P, C.POINTER(gd_cache_stats)]),
        "gd_cache_entries": (C.c_int, [P, P, P, P, P, U64, C.POINTER(U64)]),
        "gd_cache_add_ext": (C.c_int, [P, P, C.POINTER(gd_key_ext), P, P, U32]),
        "gd_cache_remove_ext": (C.c_int, [P, P, C.POINTER(gd_key_ext), U32, P]),
        "gd_cache_lookup_ext": (C.c_int, [P, P, C.POINTER(gd_key_ext), U32, P, P, P]),
        "gd_cache_entries_ext": (C.c_int, [P, P, P, P, P, P, P, P, U64, U64, C.POINTER(U64), C.POINTER(U64)]),
        "gd_dir_register_ext": (C.c_int, [P, P, C.POINTER(gd_key_ext), P, U32, P, P]),
        "gd_dir_unregister_ext": (C.c_int, [P, P, C.POINTER(gd_key_ext), P, U32, P]),
        "gd_dir_lookup_ext": (C.c_int, [P, P, C.POINTER(gd_key_ext), U32, P, P]),
        "gd_uniform_hashes_ext": (C.c_int, [P, P, C.POINTER(gd_key_ext), U32, P]),
        "gd_dir_ext_stats": (C.c_int, [P, C.POINTER(U64), C.POINTER(U64), C.POINTER(U64)]),
        "gd_route_ext": (C.c_int, [P, P, C.POINTER(gd_key_ext), U32, P, P, P]),
        "gd_route_bucket_ext": (C.c_int, [P, P, C.POINTER(gd_key_ext), U32, U32, P, P, P, P, P]),
        "gd_route_ext_device": (C.c_int, [P, P, C.POINTER(gd_key_ext), U32, P, P, P]),
        "gd_route_bucket_ext_device": (C.c_int, [P, P, C.POINTER(gd_key_ext), U32, U32, P, P, P, P, P]),
        "gd_comm_unique_id": (C.c_int, [P]),
        "gd_comm_init": (C.c_int, [P, P, C.c_int, C.c_int]),
        "gd_comm_init_local": (C.c_int, [P, C.c_int]),
        "gd_comm_destroy": (C.c_int, [P]),
        "gd_route_multi_device": (C.c_int, [P, P, U32, U32, C.c_int, C.POINTER(gd_multi_result)]),
        "gd_route_multi": (C.c_int, [P, P, U32, U32, C.c_int, C.POINTER(gd_multi_result)]),
        "gd_multi_fetch": (C.c_int, [P] + [P] * 11),
        "gd_route_multi_ext_device": (C.c_int, [P, P, C.POINTER(gd_key_ext), U32, U32, C.c_int,
                                                C.POINTER(gd_multi_result)]),
        "gd_ring_owner_ext": (C.c_int, [P, P, C.POINTER(gd_key_ext), U32, P]),
        "gd_dir_split_ext": (C.c_int, [P, P, U32, C.c_int, P, P, P, P, P, U64, U64, C.POINTER(U64), C.POINTER(U64)]),
        "gd_route_multi_ext": (C.c_int, [P, P, C.POINTER(gd_key_ext), U32, U32, C.c_int, C.POINTER(gd_multi_result)]),
        "gd_fanout_multi_device": (C.c_int, [P, P, P, U32, P, U32, C.c_int32, U32, U32, P]),
        "gd_fanout_multi_part_device": (C.c_int, [P, P, P, U32, P, P, U32, C.c_int32, U32, P]),
        "gd_fanout_cascade_device": (C.c_int, [P, P, P, U32, P, U32, C.c_int32, U32, U32, P]),
        "gd_fanout_multi": (C.c_int, [P, P, P, U32, P, U32, C.c_int32, U32, U32, P]),
        "gd_fanout_multi_fetch": (C.c_int, [P, U32] + [P] * 9),
        "gd_dir_handoff_multi": (C.c_int, [P, P, U32, C.c_int, U32, C.POINTER(gd_handoff_result)]),
        "gd_dir_handoff_fetch": (C.c_int, [P] + [P] * 7),
        "gd_option_set": (C.c_int, [P, C.c_int, C.c_int64]),
        "gd_option_get": (C.c_int, [P, C.c_int, C.POINTER(C.c_int64)]),
        "gd_tune_reset": (C.c_int, [P]),
        "gd_tune_set": (C.c_int, [P, C.c_int, C.c_int]),
        "gd_tune_get": (C.c_int, [P, C.c_int, U64, U32, C.POINTER(C.c_int)]),
        "gd_tune_agree": (C.c_int, [P]),
        "gd_comm_info": (C.c_int, [P, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    }
    ab_variant = "GRAINDISPATCH_LIB" in os.environ     # an older build for an A/B: its missing entry points stay unbound
    for name, (res, args) in sig.items():
        fn = getattr(lib, name, None)
        if fn is None and ab_variant:
            continue
        if fn is None:
            raise ImportError(f"{LIB_PATH} lacks {name}: rebuild it (__graft_entry__.build())")
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def _ptr(a: np.ndarray) -> int:
    return a.ctypes.data


def keys_array(keys) -> np.ndarray:
    """(N,3) uint64 [n0, n1, type_code_data] in C order (the gd_key AoS layout)."""
    k = np.ascontiguousarray(np.asarray(keys, dtype=np.uint64).reshape(-1, 3))
    return k


# ---- identity helpers ------------------------------------------------------------

def silo_addr(ip: str, port: int, gen: int) -> gd_silo_addr:
    import ipaddress
    a = ipaddress.ip_address(ip)
    s = gd_silo_addr()
    raw = (b"\x00" * 12 + a.packed) if a.version == 4 else a.packed
    for i, b in enumerate(raw):
        s.ip[i] = b
    s.port, s.generation, s.is_v4 = port, gen, 1 if a.version == 4 else 0
    return s


def jenkins_bytes(data: bytes) -> int:
    buf = (C.c_uint8 * max(1, len(data))).from_buffer_copy(data or b"\0")
    return lib.gd_jenkins_hash_bytes(buf, len(data))


def jenkins_u64x3(u1: int, u2: int, u3: int) -> int:
    return lib.gd_jenkins_hash_u64x3(u1, u2, u3)


def calculate_id_hash(text: str) -> int:
    return lib.gd_calculate_id_hash(text.encode("utf-8"))


def silo_consistent_hash(ip: str, port: int, gen: int) -> int:
    return lib.gd_silo_consistent_hash(C.byref(silo_addr(ip, port, gen)))


def silo_uniform_hashes(ip: str, port: int, gen: int, n: int) -> List[int]:
    out = np.zeros(max(n, 1), dtype=np.uint32)
    _check(None, lib.gd_silo_uniform_hashes(C.byref(silo_addr(ip, port, gen)), n, _ptr(out)))
    return [int(x) for x in out[:n]]


def ring_build(mode: str, silos: Sequence[Tuple[str, int, int]], buckets: int = 30) -> Tuple[np.ndarray, np.ndarray]:
    """LocalGrainDirectory / ConsistentRingProvider / VirtualBucketsRingProvider
    AddServer over `silos` (added in order).  Returns (points u32, owner u32)."""
    m = RING_MODES[mode] if isinstance(mode, str) else mode
    arr = (gd_silo_addr * len(silos))(*[silo_addr(*s) for s in silos])
    cap = len(silos) * (buckets if m == RING_VIRTUAL_BUCKETS else 1)
    pts = np.zeros(cap, dtype=np.uint32)
    own = np.zeros(cap, dtype=np.uint32)
    n = C.c_uint32(0)
    _check(None, lib.gd_ring_build(m, arr, len(silos), buckets, _ptr(pts), _ptr(own), C.byref(n)))
    return pts[: n.value].copy(), own[: n.value].copy()


def _check(h, rc: int):
    if rc != GD_OK:
        msg = lib.gd_last_error(h)
        raise GrainDispatchError(rc, msg.decode() if msg else "")


# ---- handle options (include/graindispatch.h GD_OPT_*) and measured choices (GD_TUNE_*) -----------
OPTIONS = {"probe": 1, "bucket": 2, "l2_small": 3, "stable_rank": 4, "wire_headers": 5, "region_probe": 6,
           "idx16": 7, "host_chunk": 8, "mb_zerocopy": 9, "mb_split": 10, "mb_trace": 11, "l2_staged": 12,
           "l2_mid": 13, "b2_persist": 14, "b2_order": 15, "mb_poll": 16,
           "fan_bound": 17}
# GD_OPT_WALK_INVALIDATION: set_option / get_option take it by number (OPTIONS names the options whose defaults
# the configuration tests enumerate)
OPT_WALK_INVALIDATION = 18
TUNE_KINDS = {"probe_keys": 0, "probe_n1": 1, "probe_fanout": 2, "probe_nodes": 3, "bucket": 4}
# Options applied to every handle this process creates, before its own `options=` (the test and tool
# harness sets these; a C# host calls gd_option_set on its handle instead).
DEFAULT_OPTIONS: dict = {}
# Every handle created as if its device failed gd_create's lane-order check (GD_CFG_NO_LANE_ORDER): the
# test suite's ballot-rank run (tests/conftest.py, GD_TEST_BALLOT_RANKS=1) sets it
FORCE_NO_LANE_ORDER = False


# ---- the handle --------------------------------------------------------------------

class GrainDispatch:
    """One libgraindispatch handle: a ring snapshot + the directory partitions this
    GPU owns + scratch, on one HIP stream."""

    def __init__(self, device: int = 0, table_capacity: int = 1 << 20, my_silo: int = 0,
                 seed_silo: int = NO_SILO, kernel_timing: bool = False, options: Optional[dict] = None,
                 no_lane_order: bool = False):
        """no_lane_order (GD_CFG_NO_LANE_ORDER): the handle behaves as on a device that fails gd_create's
        LDS lane-order check -- every stable rank by ballots."""
        cfg = gd_config(C.sizeof(gd_config), device, table_capacity, my_silo, seed_silo, 0,
                        (CFG_KERNEL_TIMING if kernel_timing else 0) |
                        (CFG_NO_LANE_ORDER if no_lane_order or FORCE_NO_LANE_ORDER else 0))
        h = C.c_void_p()
        _check(None, lib.gd_create(C.byref(cfg), C.byref(h)))
        self.h = h
        self.device = device
        for k, v in {**DEFAULT_OPTIONS, **(options or {})}.items():
            self.set_option(k, v)

    # -- options and measured choices ------------------------------------------
    def set_option(self, name, value: int):
        self._c(lib.gd_option_set(self.h, OPTIONS[name] if isinstance(name, str) else name, int(value)))

    def get_option(self, name) -> int:
        v = C.c_int64(0)
        self._c(lib.gd_option_get(self.h, OPTIONS[name] if isinstance(name, str) else name, C.byref(v)))
        return v.value

    def tune_reset(self):
        self._c(lib.gd_tune_reset(self.h))

    def tune_set(self, kind, variant: int):
        self._c(lib.gd_tune_set(self.h, TUNE_KINDS[kind] if isinstance(kind, str) else kind, variant))

    def tune_get(self, kind, n: int, sub: int = 0) -> int:
        v = C.c_int(0)
        self._c(lib.gd_tune_get(self.h, TUNE_KINDS[kind] if isinstance(kind, str) else kind, n, sub, C.byref(v)))
        return v.value

    def tune_agree(self):
        """Collective over the handle's communicator: every rank keeps the same measured choices."""
        self._c(lib.gd_tune_agree(self.h))

    def comm_info(self) -> dict:
        """{"n_ranks", "rank", "transport"} of the handle's communicator (RCCL's own count)."""
        nr, rk, tr = C.c_int(0), C.c_int(0), C.c_int(0)
        self._c(lib.gd_comm_info(self.h, C.byref(nr), C.byref(rk), C.byref(tr)))
        return {"n_ranks": nr.value, "rank": rk.value,
                "transport": {0: "none", 1: "rccl", 2: "in-process"}.get(tr.value, str(tr.value))}

    def close(self):
        if getattr(self, "h", None):
            lib.gd_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def _c(self, rc):
        _check(self.h, rc)

    # -- stream ---------------------------------------------------------------
    def set_stream(self, hip_stream: Optional[int]):
        self._c(lib.gd_set_stream(self.h, C.c_void_p(hip_stream or 0)))

    def set_bucket_stream(self, hip_stream: Optional[int]):
        """gd_set_bucket_stream: route_bucket_device's bucketing on this stream, after the route."""
        self._c(lib.gd_set_bucket_stream(self.h, C.c_void_p(hip_stream or 0)))

    def synchronize(self):
        self._c(lib.gd_synchronize(self.h))

    def stats(self) -> dict:
        s = gd_stats()
        self._c(lib.gd_stats_get(self.h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in gd_stats._fields_}

    def index_stats(self) -> dict:
        """gd_index_stats_get: builds, slots re-projected by directory batches, the 8-B layout."""
        s = gd_index_stats()
        self._c(lib.gd_index_stats_get(self.h, C.byref(s)))
        return {f: getattr(s, f) for f, _ in gd_index_stats._fields_}

    # -- ring -----------------------------------------------------------------
    def ring_set(self, mode, points, owner):
        m = RING_MODES[mode] if isinstance(mode, str) else mode
        p = np.ascontiguousarray(np.asarray(points, dtype=np.int64).astype(np.uint32) if np.asarray(points).dtype.kind == "i"
                                 else np.asarray(points, dtype=np.uint32))
        o = np.ascontiguousarray(np.asarray(owner, dtype=np.uint32))
        self._c(lib.gd_ring_set(self.h, m, _ptr(p), _ptr(o), len(p)))

    def ring_set_silos(self, mode: str, silos, buckets: int = 30):
        pts, own = ring_build(mode, silos, buckets)
        self.ring_set(mode, pts, own)
        return pts, own

    def ring_owner(self, keys) -> np.ndarray:
        k = keys_array(keys)
        out = np.zeros(len(k), dtype=np.uint32)
        self._c(lib.gd_ring_owner(self.h, _ptr(k), len(k), _ptr(out)))
        return out

    def ring_lookup_hashes(self, hashes) -> np.ndarray:
        hs = np.ascontiguousarray(np.asarray(hashes, dtype=np.uint32))
        out = np.zeros(len(hs), dtype=np.uint32)
        self._c(lib.gd_ring_lookup_hashes(self.h, _ptr(hs), len(hs), _ptr(out)))
        return out

    # -- directory ------------------------------------------------------------
    def register(self, keys, acts, silos):
        k = keys_array(keys)
        n = len(k)
        vals = np.zeros((n, 2), dtype=np.uint32)
        vals[:, 0] = acts
        vals[:, 1] = silos
        out = np.zeros((n, 2), dtype=np.uint32)
        ins = np.zeros(n, dtype=np.uint8)
        self._c(lib.gd_dir_register(self.h, _ptr(k), _ptr(vals), n, _ptr(out), _ptr(ins)))
        return out[:, 0].copy(), out[:, 1].copy(), ins

    def register_device(self, d_keys: int, d_vals: int, n: int, d_out_vals: Optional[int] = None,
                        d_out_inserted: Optional[int] = None):
        """gd_dir_register_device: keys (n,3) u64 and values (n,2) u32 [act, silo] in HBM."""
        self._c(lib.gd_dir_register_device(self.h, C.c_void_p(d_keys), C.c_void_p(d_vals), n,
                                           C.c_void_p(d_out_vals or 0), C.c_void_p(d_out_inserted or 0)))

    def register_device_async(self, d_keys: int, d_vals: int, n: int, d_out_vals: Optional[int] = None,
                              d_out_inserted: Optional[int] = None):
        """gd_dir_register_device_async: enqueued only (device errors at the next synchronising call)."""
        self._c(lib.gd_dir_register_device_async(self.h, C.c_void_p(d_keys), C.c_void_p(d_vals), n,
                                                 C.c_void_p(d_out_vals or 0), C.c_void_p(d_out_inserted or 0)))

    def unregister_device(self, d_keys: int, d_acts: int, n: int, d_out_removed: Optional[int] = None):
        """gd_dir_unregister_device: RemoveActivation over device arrays, enqueued only."""
        self._c(lib.gd_dir_unregister_device(self.h, C.c_void_p(d_keys), C.c_void_p(d_acts), n,
                                             C.c_void_p(d_out_removed or 0)))

    # -- membership change: IsValidSilo, VersionTag, silo removal, merge ----------
    def set_valid_silos(self, valid_silos, n_silos: int):
        """gd_dir_set_valid_silos: the silos of [0, n_silos) that are valid (IsValidSilo); n_silos 0 =
        every silo valid."""
        m = np.zeros(max(n_silos, 1), dtype=np.uint8)
        if n_silos:
            m[[int(x) for x in valid_silos]] = 1
        self._c(lib.gd_dir_set_valid_silos(self.h, _ptr(m), n_silos))

    def lookup_tagged(self, keys):
        """LookUpActivations with VersionTag: (act, silo, tag i32, found u8: 0 absent, 1 valid, 2 invalid silo)."""
        k = keys_array(keys)
        n = len(k)
        vals = np.zeros((n, 2), np.uint32)
        tags = np.zeros(n, np.int32)
        found = np.zeros(n, np.uint8)
        self._c(lib.gd_dir_lookup_tagged(self.h, _ptr(k), n, _ptr(vals), _ptr(tags), _ptr(found)))
        return vals[:, 0].copy(), vals[:, 1].copy(), tags, found

    def remove_silos(self, silos) -> dict:
        """AdjustLocalDirectory (+ AdjustLocalCache in LocalLookup mode) for removed silos."""
        a = np.ascontiguousarray(np.asarray(list(silos), dtype=np.uint32))
        r, m, c = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._c(lib.gd_dir_remove_silos(self.h, _ptr(a) if len(a) else None, len(a), C.byref(r), C.byref(m),
                                        C.byref(c)))
        return {"removed": r.value, "multi": m.value, "cache_removed": c.value}

    def activation_ids_set(self, acts, ids):
        a = np.ascontiguousarray(np.asarray(acts, dtype=np.uint32))
        k = keys_array(ids)
        self._c(lib.gd_activation_ids_set(self.h, _ptr(a), _ptr(k), len(a)))

    def merge(self, keys, acts, silos, tags=None):
        """gd_dir_merge: (status u8, dropped act u32, dropped silo u32)."""
        k = keys_array(keys)
        n = len(k)
        vals = np.zeros((n, 2), np.uint32)
        vals[:, 0] = acts
        vals[:, 1] = silos
        t = None if tags is None else np.ascontiguousarray(np.asarray(tags, dtype=np.int32))
        st = np.zeros(n, np.uint8)
        dr = np.zeros((n, 2), np.uint32)
        self._c(lib.gd_dir_merge(self.h, _ptr(k), _ptr(vals), None if t is None else _ptr(t), n, _ptr(st), _ptr(dr)))
        return st, dr[:, 0].copy(), dr[:, 1].copy()

    # -- receive path: ActivationDirectory + IncomingMessageAgent ------------------
    def actdir_add(self, ids, ctx, flags) -> np.ndarray:
        k = keys_array(ids)
        c = np.ascontiguousarray(np.asarray(ctx, dtype=np.uint32))
        f = np.ascontiguousarray(np.asarray(flags, dtype=np.uint8))
        out = np.zeros(len(k), np.uint8)
        self._c(lib.gd_actdir_add(self.h, _ptr(k), _ptr(c), _ptr(f), len(k), _ptr(out)))
        return out

    def actdir_remove(self, ids) -> np.ndarray:
        k = keys_array(ids)
        out = np.zeros(len(k), np.uint8)
        self._c(lib.gd_actdir_remove(self.h, _ptr(k), len(k), _ptr(out)))
        return out

    def actdir_set_flags(self, ids, flags) -> np.ndarray:
        k = keys_array(ids)
        f = np.ascontiguousarray(np.asarray(flags, dtype=np.uint8))
        out = np.zeros(len(k), np.uint8)
        self._c(lib.gd_actdir_set_flags(self.h, _ptr(k), _ptr(f), len(k), _ptr(out)))
        return out

    def actdir_lookup(self, ids):
        k = keys_array(ids)
        n = len(k)
        c = np.zeros(n, np.uint32)
        f = np.zeros(n, np.uint8)
        found = np.zeros(n, np.uint8)
        self._c(lib.gd_actdir_lookup(self.h, _ptr(k), n, _ptr(c), _ptr(f), _ptr(found)))
        return c, f, found

    def actdir_clear(self):
        self._c(lib.gd_actdir_clear(self.h))

    def actdir_count(self) -> int:
        v = C.c_uint64()
        self._c(lib.gd_actdir_count(self.h, C.byref(v)))
        return v.value

    @staticmethod
    def _limits(request_count, hard_limit, hard_limit_sw):
        if request_count is None:
            return None, None
        rc = np.ascontiguousarray(np.asarray(request_count, dtype=np.uint32))
        return gd_recv_limits(_ptr(rc), hard_limit, hard_limit_sw), rc

    def receive(self, target_grain, target_activation, direction, n_ctx: int, request_count=None, hard_limit: int = 0,
                hard_limit_sw: int = 0, bucket: bool = True):
        """gd_receive: (ctx u32, status u8[, perm, offsets[n_ctx + 3]])."""
        tg = keys_array(target_grain)
        ta = keys_array(target_activation)
        n = len(tg)
        d = None if direction is None else np.ascontiguousarray(np.asarray(direction, dtype=np.uint8))
        lim, keep = self._limits(request_count, hard_limit, hard_limit_sw)
        ctx = np.zeros(n, np.uint32)
        st = np.zeros(n, np.uint8)
        perm = np.zeros(n, np.uint32) if bucket else None
        off = np.zeros(n_ctx + 3, np.uint32) if bucket else None
        self._c(lib.gd_receive(self.h, _ptr(tg), _ptr(ta), None if d is None else _ptr(d), n, n_ctx,
                               None if lim is None else C.byref(lim), _ptr(ctx), _ptr(st),
                               None if perm is None else _ptr(perm), None if off is None else _ptr(off)))
        return (ctx, st, perm, off) if bucket else (ctx, st)

    def receive_frames(self, buf: bytes, offsets, n_ctx: int, request_count=None, hard_limit: int = 0,
                       hard_limit_sw: int = 0, fields: Optional[Iterable[str]] = ()):
        """gd_receive_frames: (decoded fields, ctx, status, perm, offsets)."""
        b = np.frombuffer(buf, dtype=np.uint8) if len(buf) else np.zeros(1, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        n = len(off)
        arrs, ff = self._frame_host(n, fields)
        lim, keep = self._limits(request_count, hard_limit, hard_limit_sw)
        ctx = np.zeros(n, np.uint32)
        st = np.zeros(n, np.uint8)
        perm = np.zeros(n, np.uint32)
        offs = np.zeros(n_ctx + 3, np.uint32)
        self._c(lib.gd_receive_frames(self.h, _ptr(b), len(buf), _ptr(off), n, n_ctx,
                                      None if lim is None else C.byref(lim), C.byref(ff), _ptr(ctx), _ptr(st),
                                      _ptr(perm), _ptr(offs)))
        return arrs, ctx, st, perm, offs

    def receive_device(self, d_tg: int, d_ta: int, d_dir: Optional[int], n: int, n_ctx: int, d_ctx: int, d_status: int,
                       d_perm: Optional[int], d_offsets: Optional[int], d_request_count: Optional[int] = None,
                       hard_limit: int = 0, hard_limit_sw: int = 0):
        lim = gd_recv_limits(d_request_count, hard_limit, hard_limit_sw) if d_request_count else None
        self._c(lib.gd_receive_device(self.h, C.c_void_p(d_tg), C.c_void_p(d_ta), C.c_void_p(d_dir or 0), n, n_ctx,
                                      None if lim is None else C.byref(lim), C.c_void_p(d_ctx), C.c_void_p(d_status),
                                      C.c_void_p(d_perm or 0), C.c_void_p(d_offsets or 0)))

    # -- sender queues (OutboundMessageQueue.SendMessage) ----------------------------------
    def send_configure(self, silo_hash, n_queues: int):
        """gd_send_configure: silo_hash[s] = SiloAddress.GetConsistentHashCode of silo index s."""
        sh = np.ascontiguousarray(np.asarray(silo_hash, dtype=np.int32))
        self._c(lib.gd_send_configure(self.h, _ptr(sh), len(sh), n_queues))
        self.send_n_queues = n_queues

    @staticmethod
    def _opt(a, dtype):
        return None if a is None else np.ascontiguousarray(np.asarray(a, dtype=dtype))

    def send_queues(self, silo, route_status=None, category=None, ttl=None, bucket: bool = True):
        """gd_send_queues: (send_status u8, queue u32[, perm, offsets[n_queues + 5]])."""
        s = np.ascontiguousarray(np.asarray(silo, dtype=np.uint32))
        n = len(s)
        rs, cat, tl = self._opt(route_status, np.uint8), self._opt(category, np.uint8), self._opt(ttl, np.int64)
        st = np.zeros(n, np.uint8)
        q = np.zeros(n, np.uint32)
        perm = np.zeros(n, np.uint32) if bucket else None
        off = np.zeros(self.send_n_queues + 5, np.uint32) if bucket else None
        self._c(lib.gd_send_queues(self.h, _ptr(s), None if rs is None else _ptr(rs), None if cat is None else _ptr(cat),
                                   None if tl is None else _ptr(tl), n, _ptr(st), _ptr(q),
                                   None if perm is None else _ptr(perm), None if off is None else _ptr(off)))
        return (st, q, perm, off) if bucket else (st, q)

    def send_queues_device(self, d_silo: int, d_route_status: Optional[int], d_category: Optional[int],
                           d_ttl: Optional[int], n: int, d_send_status: int, d_queue: Optional[int],
                           d_perm: Optional[int], d_offsets: Optional[int]):
        self._c(lib.gd_send_queues_device(self.h, C.c_void_p(d_silo), C.c_void_p(d_route_status or 0),
                                          C.c_void_p(d_category or 0), C.c_void_p(d_ttl or 0), n,
                                          C.c_void_p(d_send_status), C.c_void_p(d_queue or 0), C.c_void_p(d_perm or 0),
                                          C.c_void_p(d_offsets or 0)))

    def route_send(self, keys, category=None, ttl=None):
        """gd_route_send: (status, silo, act, send_status, queue, perm, offsets[n_queues + 5])."""
        k = keys_array(keys)
        n = len(k)
        cat, tl = self._opt(category, np.uint8), self._opt(ttl, np.int64)
        silo = np.zeros(n, np.uint32)
        act = np.zeros(n, np.uint32)
        st = np.zeros(n, np.uint8)
        sst = np.zeros(n, np.uint8)
        q = np.zeros(n, np.uint32)
        perm = np.zeros(n, np.uint32)
        off = np.zeros(self.send_n_queues + 5, np.uint32)
        self._c(lib.gd_route_send(self.h, _ptr(k), n, None if cat is None else _ptr(cat),
                                  None if tl is None else _ptr(tl), _ptr(silo), _ptr(act), _ptr(st), _ptr(sst), _ptr(q),
                                  _ptr(perm), _ptr(off)))
        return st, silo, act, sst, q, perm, off

    def route_send_device(self, d_keys: int, n: int, d_category: Optional[int], d_ttl: Optional[int], d_silo: int,
                          d_act: int, d_status: int, d_send_status: int, d_queue: Optional[int],
                          d_perm: Optional[int], d_offsets: Optional[int]):
        self._c(lib.gd_route_send_device(self.h, C.c_void_p(d_keys), n, C.c_void_p(d_category or 0),
                                         C.c_void_p(d_ttl or 0), C.c_void_p(d_silo), C.c_void_p(d_act),
                                         C.c_void_p(d_status), C.c_void_p(d_send_status), C.c_void_p(d_queue or 0),
                                         C.c_void_p(d_perm or 0), C.c_void_p(d_offsets or 0)))

    # -- placement of unregistered grains (Dispatcher.AddressMessageAsync's slow path) -----------
    def place_configure(self, silos: Sequence[Tuple[str, int, int]], compatible=None, local_active: bool = True):
        """gd_place_configure: the silo table [(ip, port, generation)], compatible flags (None = all)."""
        arr = (gd_silo_addr * max(1, len(silos)))(*[silo_addr(*s) for s in silos])
        c = self._opt(compatible, np.uint8)
        self._c(lib.gd_place_configure(self.h, arr, len(silos), None if c is None else _ptr(c), int(local_active)))

    def route_place(self, keys, act_base: int, strategy=PLACE_HASH, given_silo=None):
        """gd_route_place: (status, silo, act, placed u8, new_idx u32[n_new], n_proposed).  strategy: one
        GD_PLACE_* value for the batch, or a u8 array with one a message."""
        return self._route_place(keys, act_base, strategy, given_silo, None)

    def route_place_bucket(self, keys, n_act: int, act_base: int, strategy=PLACE_HASH, given_silo=None):
        """gd_route_place_bucket: (status, silo, act, placed, new_idx, n_proposed, perm, offsets[n_act + 2])."""
        return self._route_place(keys, act_base, strategy, given_silo, n_act)

    def _route_place(self, keys, act_base, strategy, given_silo, n_act):
        k = keys_array(keys)
        n = len(k)
        per = None if np.isscalar(strategy) else np.ascontiguousarray(np.asarray(strategy, dtype=np.uint8))
        dflt = int(strategy) if per is None else PLACE_NONE
        gv = self._opt(given_silo, np.uint32)
        silo = np.zeros(n, np.uint32)
        act = np.zeros(n, np.uint32)
        st = np.zeros(n, np.uint8)
        placed = np.zeros(n, np.uint8)
        new_idx = np.zeros(max(n, 1), np.uint32)
        n_new, n_prop = C.c_uint32(0), C.c_uint32(0)
        head = (self.h, _ptr(k), n, None if per is None else _ptr(per), dflt, None if gv is None else _ptr(gv),
                act_base, _ptr(silo), _ptr(act), _ptr(st), _ptr(placed), _ptr(new_idx), C.byref(n_new), C.byref(n_prop))
        if n_act is None:
            self._c(lib.gd_route_place(*head))
            return st, silo, act, placed, new_idx[:n_new.value].copy(), n_prop.value
        perm = np.zeros(n, np.uint32)
        off = np.zeros(n_act + 2, np.uint32)
        self._c(lib.gd_route_place_bucket(*head, n_act, _ptr(perm), _ptr(off)))
        return st, silo, act, placed, new_idx[:n_new.value].copy(), n_prop.value, perm, off

    def route_place_device(self, d_keys: int, n: int, d_strategy: Optional[int], default_strategy: int,
                           d_given_silo: Optional[int], act_base: int, d_silo: int, d_act: int, d_status: int,
                           d_placed: int, d_new_idx: Optional[int], n_act: Optional[int] = None,
                           d_perm: Optional[int] = None, d_offsets: Optional[int] = None) -> Tuple[int, int]:
        """gd_route_place_device, or gd_route_place_bucket_device when n_act is given: (n_new, n_proposed)."""
        n_new, n_prop = C.c_uint32(0), C.c_uint32(0)
        head = (self.h, C.c_void_p(d_keys), n, C.c_void_p(d_strategy or 0), default_strategy,
                C.c_void_p(d_given_silo or 0), act_base, C.c_void_p(d_silo), C.c_void_p(d_act), C.c_void_p(d_status),
                C.c_void_p(d_placed), C.c_void_p(d_new_idx or 0), C.byref(n_new), C.byref(n_prop))
        if n_act is None:
            self._c(lib.gd_route_place_device(*head))
        else:
            self._c(lib.gd_route_place_bucket_device(*head, n_act, C.c_void_p(d_perm or 0), C.c_void_p(d_offsets or 0)))
        return n_new.value, n_prop.value

    # -- turn admission of a received batch (Dispatcher.ReceiveRequest) --------------------------
    def turns(self, ctx, n_ctx: int, ctx_flags, num_running, request_count, recv_status=None, direction=None,
              ttl=None, forward_count=None, msg_flags=None, target_activation=None, sending_activation=None,
              hard_limit: int = 0, hard_limit_sw: int = 0, max_forward_count: int = 2, chain: bool = False,
              lists: bool = True):
        """gd_turns: (turn u8, num_running_out u32[n_ctx], running_idx u32[n_ctx][, start_idx u32[n_start],
        wait_perm u32[n], wait_offsets u32[n_ctx + 2]])."""
        c = np.ascontiguousarray(np.asarray(ctx, dtype=np.uint32))
        n = len(c)
        rs, dr, tl = self._opt(recv_status, np.uint8), self._opt(direction, np.uint8), self._opt(ttl, np.int64)
        fw, mf = self._opt(forward_count, np.uint8), self._opt(msg_flags, np.uint8)
        ta = None if target_activation is None else keys_array(target_activation)
        sa = None if sending_activation is None else keys_array(sending_activation)
        fl, nr = self._opt(ctx_flags, np.uint8), self._opt(num_running, np.uint32)
        rc = self._opt(request_count, np.uint32)
        st = gd_turn_state(None if fl is None else _ptr(fl), None if nr is None else _ptr(nr),
                           None if rc is None else _ptr(rc), hard_limit, hard_limit_sw, max_forward_count, int(chain))
        turn = np.zeros(n, np.uint8)
        nro = np.zeros(n_ctx, np.uint32)
        run = np.zeros(n_ctx, np.uint32)
        start = np.zeros(max(n, 1), np.uint32) if lists else None
        n_start = np.zeros(1, np.uint32) if lists else None
        perm = np.zeros(n, np.uint32) if lists else None
        off = np.zeros(n_ctx + 2, np.uint32) if lists else None
        p = lambda a: None if a is None else _ptr(a)
        self._c(lib.gd_turns(self.h, _ptr(c), p(rs), p(dr), p(tl), p(fw), p(mf), p(ta), p(sa), n, n_ctx, C.byref(st),
                             _ptr(turn), _ptr(nro), _ptr(run), p(start), p(n_start), p(perm), p(off)))
        if not lists:
            return turn, nro, run
        return turn, nro, run, start[:int(n_start[0])].copy(), perm, off

    @staticmethod
    def turn_state_device(d_ctx_flags: int, d_num_running: int, d_request_count: Optional[int] = None,
                          hard_limit: int = 0, hard_limit_sw: int = 0, max_forward_count: int = 2,
                          chain: bool = False) -> gd_turn_state:
        return gd_turn_state(d_ctx_flags or None, d_num_running or None, d_request_count or None, hard_limit,
                             hard_limit_sw, max_forward_count, int(chain))

    def turns_device(self, d_ctx: int, d_recv_status: Optional[int], d_direction: Optional[int], d_ttl: Optional[int],
                     d_forward_count: Optional[int], d_msg_flags: Optional[int], d_target_activation: Optional[int],
                     d_sending_activation: Optional[int], n: int, n_ctx: int, state: gd_turn_state, d_turn: int,
                     d_num_running_out: int, d_running_idx: int, d_start_idx: Optional[int] = None,
                     d_n_start: Optional[int] = None, d_wait_perm: Optional[int] = None,
                     d_wait_offsets: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_turns_device(self.h, V(d_ctx), V(d_recv_status), V(d_direction), V(d_ttl), V(d_forward_count),
                                    V(d_msg_flags), V(d_target_activation), V(d_sending_activation), n, n_ctx,
                                    C.byref(state), V(d_turn), V(d_num_running_out), V(d_running_idx), V(d_start_idx),
                                    V(d_n_start), V(d_wait_perm), V(d_wait_offsets)))

    def receive_turns_device(self, d_tg: int, d_ta: int, d_dir: Optional[int], n: int, n_ctx: int, d_ctx: int,
                             d_status: int, d_perm: Optional[int], d_offsets: Optional[int], d_ttl: Optional[int],
                             d_forward_count: Optional[int], d_msg_flags: Optional[int],
                             d_sending_activation: Optional[int], state: gd_turn_state, d_turn: int,
                             d_num_running_out: int, d_running_idx: int, d_start_idx: Optional[int] = None,
                             d_n_start: Optional[int] = None, d_wait_perm: Optional[int] = None,
                             d_wait_offsets: Optional[int] = None, d_recv_request_count: Optional[int] = None,
                             recv_hard_limit: int = 0, recv_hard_limit_sw: int = 0):
        V = lambda x: C.c_void_p(x or 0)
        lim = gd_recv_limits(d_recv_request_count, recv_hard_limit, recv_hard_limit_sw) if d_recv_request_count else None
        self._c(lib.gd_receive_turns_device(self.h, V(d_tg), V(d_ta), V(d_dir), n, n_ctx,
                                            None if lim is None else C.byref(lim), V(d_ctx), V(d_status), V(d_perm),
                                            V(d_offsets), V(d_ttl), V(d_forward_count), V(d_msg_flags),
                                            V(d_sending_activation), C.byref(state), V(d_turn), V(d_num_running_out),
                                            V(d_running_idx), V(d_start_idx), V(d_n_start), V(d_wait_perm),
                                            V(d_wait_offsets)))

    # -- the frame-fed chain: receive buffer -> decode -> ReceiveMessage -> ReceiveRequest ----------
    @staticmethod
    def _frame_turn_host(n: int, turn_fields) -> Tuple[dict, Optional[gd_frame_turn_fields]]:
        """turn_fields: None = no struct (NULL), else the members wanted (an empty list: a struct of NULLs)."""
        if turn_fields is None:
            return {}, None
        arrs = {k: np.zeros(n, dtype=FRAME_TURN_FIELDS[k]) for k in turn_fields}
        return arrs, gd_frame_turn_fields(**{k: (_ptr(a) if n else None) for k, a in arrs.items()})

    def decode_frames_turn(self, buf: bytes, offsets, fields: Optional[Iterable[str]] = None,
                           turn_fields: Optional[Iterable[str]] = tuple(FRAME_TURN_FIELDS)):
        """gd_decode_frames_turn: (decoded fields, decoded turn headers), dicts of numpy arrays named like
        gd_frame_fields / gd_frame_turn_fields.  turn_fields None passes a NULL struct."""
        b = np.frombuffer(buf, dtype=np.uint8) if len(buf) else np.zeros(1, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        n = len(off)
        arrs, ff = self._frame_host(n, fields)
        tarrs, tf = self._frame_turn_host(n, turn_fields)
        self._c(lib.gd_decode_frames_turn(self.h, _ptr(b), len(buf), _ptr(off), n, C.byref(ff),
                                          None if tf is None else C.byref(tf)))
        return arrs, tarrs

    def decode_frames_turn_device(self, d_buf: int, buf_len: int, d_offsets: int, n: int, d_fields: dict,
                                  d_turn_fields: Optional[dict]):
        ff = gd_frame_fields(**{k: C.c_void_p(v) for k, v in d_fields.items()})
        tf = None if d_turn_fields is None else gd_frame_turn_fields(**{k: C.c_void_p(v)
                                                                        for k, v in d_turn_fields.items()})
        self._c(lib.gd_decode_frames_turn_device(self.h, C.c_void_p(d_buf), buf_len, C.c_void_p(d_offsets), n,
                                                 C.byref(ff), None if tf is None else C.byref(tf)))

    def receive_turns_frames(self, buf: bytes, offsets, n_ctx: int, ctx_flags, num_running, request_count,
                             recv_request_count=None, recv_hard_limit: int = 0, recv_hard_limit_sw: int = 0,
                             ttl_age_ticks: int = 0, msg_flags_or=None, hard_limit: int = 0, hard_limit_sw: int = 0,
                             max_forward_count: int = 2, chain: bool = False, fields: Optional[Iterable[str]] = (),
                             turn_fields: Optional[Iterable[str]] = ()):
        """gd_receive_turns_frames: (decoded fields, decoded turn headers, ctx u32, status u8, perm u32,
        offsets u32[n_ctx + 3], turn u8, num_running_out u32[n_ctx], running_idx u32[n_ctx],
        start_idx u32[n_start], wait_perm u32[n], wait_offsets u32[n_ctx + 2])."""
        b = np.frombuffer(buf, dtype=np.uint8) if len(buf) else np.zeros(1, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        n = len(off)
        arrs, ff = self._frame_host(n, fields)
        tarrs, tf = self._frame_turn_host(n, turn_fields)
        lim, keep = self._limits(recv_request_count, recv_hard_limit, recv_hard_limit_sw)
        mor = self._opt(msg_flags_or, np.uint8)
        fl, nr = self._opt(ctx_flags, np.uint8), self._opt(num_running, np.uint32)
        rc = self._opt(request_count, np.uint32)
        p = lambda a: None if a is None else _ptr(a)
        st = gd_turn_state(p(fl), p(nr), p(rc), hard_limit, hard_limit_sw, max_forward_count, int(chain))
        ctx, rst = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        perm, offs = np.zeros(n, np.uint32), np.zeros(n_ctx + 3, np.uint32)
        turn, nro, run = np.zeros(n, np.uint8), np.zeros(n_ctx, np.uint32), np.zeros(n_ctx, np.uint32)
        start, n_start = np.zeros(max(n, 1), np.uint32), np.zeros(1, np.uint32)
        wperm, woff = np.zeros(n, np.uint32), np.zeros(n_ctx + 2, np.uint32)
        self._c(lib.gd_receive_turns_frames(self.h, _ptr(b), len(buf), _ptr(off), n, n_ctx,
                                            None if lim is None else C.byref(lim), C.byref(ff),
                                            None if tf is None else C.byref(tf), _ptr(ctx), _ptr(rst), _ptr(perm),
                                            _ptr(offs), ttl_age_ticks, p(mor), C.byref(st), _ptr(turn), _ptr(nro),
                                            _ptr(run), _ptr(start), _ptr(n_start), _ptr(wperm), _ptr(woff)))
        return (arrs, tarrs, ctx, rst, perm, offs, turn, nro, run, start[:int(n_start[0])].copy(), wperm, woff)

    def receive_turns_frames_device(self, d_buf: int, buf_len: int, d_offsets: int, n: int, n_ctx: int,
                                    d_fields: Optional[dict], d_turn_fields: Optional[dict], d_ctx: int, d_status: int,
                                    d_perm: Optional[int], d_offs: Optional[int], ttl_age_ticks: int,
                                    d_msg_flags_or: Optional[int], state: gd_turn_state, d_turn: int,
                                    d_num_running_out: int, d_running_idx: int, d_start_idx: Optional[int] = None,
                                    d_n_start: Optional[int] = None, d_wait_perm: Optional[int] = None,
                                    d_wait_offsets: Optional[int] = None, d_recv_request_count: Optional[int] = None,
                                    recv_hard_limit: int = 0, recv_hard_limit_sw: int = 0):
        V = lambda x: C.c_void_p(x or 0)
        ff = None if d_fields is None else gd_frame_fields(**{k: C.c_void_p(v) for k, v in d_fields.items()})
        tf = None if d_turn_fields is None else gd_frame_turn_fields(**{k: C.c_void_p(v)
                                                                        for k, v in d_turn_fields.items()})
        lim = gd_recv_limits(d_recv_request_count, recv_hard_limit, recv_hard_limit_sw) if d_recv_request_count else None
        self._c(lib.gd_receive_turns_frames_device(
            self.h, V(d_buf), buf_len, V(d_offsets), n, n_ctx, None if lim is None else C.byref(lim),
            None if ff is None else C.byref(ff), None if tf is None else C.byref(tf), V(d_ctx), V(d_status), V(d_perm),
            V(d_offs), ttl_age_ticks, V(d_msg_flags_or), C.byref(state), V(d_turn), V(d_num_running_out),
            V(d_running_idx), V(d_start_idx), V(d_n_start), V(d_wait_perm), V(d_wait_offsets)))

    # -- turn completion and message pump (Dispatcher.OnActivationCompletedRequest) ---------------
    def turns_complete(self, done_ctx, n_ctx: int, ctx_flags, num_running, wait_offsets, wait_flags, done_flags=None,
                       wait_msg=None, started_by: bool = True, starts: bool = True, wait_cap: Optional[int] = None):
        """gd_turns_complete: (num_running_out u32[n_ctx], ctx_flags_out u8[n_ctx], n_dequeued u32[n_ctx],
        running_pos u32[n_ctx], event u8[n_ctx][, n_started_by u32[n_done]][, start_pos u32[n_start]])."""
        dc = np.ascontiguousarray(np.asarray(done_ctx, dtype=np.uint32))
        n_done = len(dc)
        df = self._opt(done_flags, np.uint8)
        fl, nr = self._opt(ctx_flags, np.uint8), self._opt(num_running, np.uint32)
        wo, wf, wm = self._opt(wait_offsets, np.uint32), self._opt(wait_flags, np.uint8), self._opt(wait_msg, np.uint32)
        p = lambda a: None if a is None else _ptr(a)
        wl = gd_wait_list(p(wo), p(wm), p(wf))
        total = int(wo[n_ctx]) if wo is not None and len(wo) > n_ctx else 0
        cap = total if wait_cap is None else wait_cap
        flo, nro = np.zeros(n_ctx, np.uint8), np.zeros(n_ctx, np.uint32)
        ndq, rpos, ev = np.zeros(n_ctx, np.uint32), np.zeros(n_ctx, np.uint32), np.zeros(n_ctx, np.uint8)
        nsb = np.zeros(n_done, np.uint32) if started_by else None
        start = np.zeros(max(cap, 1), np.uint32) if starts else None
        n_start = np.zeros(1, np.uint32) if starts else None
        self._c(lib.gd_turns_complete(self.h, _ptr(dc), p(df), n_done, n_ctx, p(fl), p(nr), C.byref(wl), cap, _ptr(flo),
                                      _ptr(nro), _ptr(ndq), _ptr(rpos), _ptr(ev), p(nsb), p(start), p(n_start)))
        out = (nro, flo, ndq, rpos, ev)
        if started_by:
            out += (nsb,)
        if starts:
            out += (start[:int(n_start[0])].copy(),)
        return out

    @staticmethod
    def wait_list_device(d_offsets: Optional[int], d_msg: Optional[int], d_flags: Optional[int]) -> gd_wait_list:
        return gd_wait_list(d_offsets or None, d_msg or None, d_flags or None)

    def turns_complete_device(self, d_done_ctx: Optional[int], d_done_flags: Optional[int], n_done: int, n_ctx: int,
                              d_ctx_flags: int, d_num_running: int, wait: gd_wait_list, wait_cap: int,
                              d_ctx_flags_out: int, d_num_running_out: int, d_n_dequeued: int, d_running_pos: int,
                              d_event: int, d_n_started_by: Optional[int] = None, d_start_pos: Optional[int] = None,
                              d_n_start: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_turns_complete_device(self.h, V(d_done_ctx), V(d_done_flags), n_done, n_ctx, V(d_ctx_flags),
                                             V(d_num_running), C.byref(wait), wait_cap, V(d_ctx_flags_out),
                                             V(d_num_running_out), V(d_n_dequeued), V(d_running_pos), V(d_event),
                                             V(d_n_started_by), V(d_start_pos), V(d_n_start)))

    def wait_list_merge(self, n_ctx: int, old_offsets, old_msg, old_flags, n_dequeued, wait_perm, wait_offsets,
                        msg_id=None, id_base: int = 0, msg_flags=None, target_activation=None, sending_activation=None,
                        chain: bool = False, cap: Optional[int] = None):
        """gd_wait_list_merge: (offsets u32[n_ctx + 1], msg u32[cap], flags u8[cap], total); the first
        min(total, cap) entries of msg / flags are written.  old_offsets None = no old list; cap None = enough."""
        oo, om, of = self._opt(old_offsets, np.uint32), self._opt(old_msg, np.uint32), self._opt(old_flags, np.uint8)
        nd = self._opt(n_dequeued, np.uint32)
        wp, wo = self._opt(wait_perm, np.uint32), self._opt(wait_offsets, np.uint32)
        n = len(wp)
        mi, mf = self._opt(msg_id, np.uint32), self._opt(msg_flags, np.uint8)
        ta = None if target_activation is None else keys_array(target_activation)
        sa = None if sending_activation is None else keys_array(sending_activation)
        p = lambda a: None if a is None else _ptr(a)
        if cap is None:
            cap = (int(oo[n_ctx]) if oo is not None else 0) + n
        old = None if oo is None else gd_wait_list(p(oo), p(om), p(of))
        off = np.zeros(n_ctx + 1, np.uint32)
        msg, flags = np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint8)
        total = np.zeros(1, np.uint32)
        self._c(lib.gd_wait_list_merge(self.h, None if old is None else C.byref(old), p(nd), n_ctx, p(wp), p(wo), n,
                                       p(mi), id_base, p(mf), p(ta), p(sa), int(chain), cap, _ptr(off), _ptr(msg),
                                       _ptr(flags), _ptr(total)))
        return off, msg[:cap], flags[:cap], int(total[0])

    def wait_list_merge_device(self, old: Optional[gd_wait_list], d_n_dequeued: Optional[int], n_ctx: int,
                               d_wait_perm: Optional[int], d_wait_offsets: int, n: int, d_msg_id: Optional[int],
                               id_base: int, d_msg_flags: Optional[int], d_target_activation: Optional[int],
                               d_sending_activation: Optional[int], chain: bool, cap: int, d_offsets_out: int,
                               d_msg_out: Optional[int], d_flags_out: Optional[int], d_total: int):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_wait_list_merge_device(self.h, None if old is None else C.byref(old), V(d_n_dequeued), n_ctx,
                                              V(d_wait_perm), V(d_wait_offsets), n, V(d_msg_id), id_base, V(d_msg_flags),
                                              V(d_target_activation), V(d_sending_activation), int(chain), cap,
                                              V(d_offsets_out), V(d_msg_out), V(d_flags_out), V(d_total)))

    # -- activation collector (Catalog/ActivationCollector.cs) --------------------------------------
    def collect_configure(self, quantum_ticks: int, now: int):
        self._c(lib.gd_collect_configure(self.h, quantum_ticks, now))

    def collect_next_ticket(self) -> int:
        out = C.c_int64(0)
        self._c(lib.gd_collect_next_ticket(self.h, C.byref(out)))
        return out.value

    @staticmethod
    def collect_state(ticket, became_idle, keep_alive_until, age_limit, flags) -> gd_collect_state:
        """A gd_collect_state over numpy arrays (int64 / uint8, contiguous: updated in place) or device addresses;
        keep_alive_until may be None."""
        p = lambda a: (a or None) if a is None or isinstance(a, int) else _ptr(a)
        for a, dt in ((ticket, np.int64), (became_idle, np.int64), (keep_alive_until, np.int64), (age_limit, np.int64),
                      (flags, np.uint8)):
            assert a is None or isinstance(a, int) or (a.dtype == dt and a.flags.c_contiguous)
        return gd_collect_state(p(ticket), p(became_idle), p(keep_alive_until), p(age_limit), p(flags))

    def collect_schedule(self, st: gd_collect_state, n_ctx: int, ctx, now: int, status: bool = True):
        """gd_collect_schedule: status u8[n] (GD_COL_SCHEDULED ...) or None; the state's arrays are updated."""
        cx = np.ascontiguousarray(np.asarray(ctx, dtype=np.uint32))
        out = np.zeros(len(cx), np.uint8) if status else None
        self._c(lib.gd_collect_schedule(self.h, C.byref(st), n_ctx, _ptr(cx), len(cx), now,
                                        None if out is None else _ptr(out)))
        return out

    def collect_cancel(self, st: gd_collect_state, n_ctx: int, ctx, cancelled: bool = True):
        cx = np.ascontiguousarray(np.asarray(ctx, dtype=np.uint32))
        out = np.zeros(len(cx), np.uint8) if cancelled else None
        self._c(lib.gd_collect_cancel(self.h, C.byref(st), n_ctx, _ptr(cx), len(cx), None if out is None else _ptr(out)))
        return out

    def collect_touch(self, st: gd_collect_state, n_ctx: int, ctx_flags, ctx, now: int, turn=None, ok: bool = True):
        """gd_collect_touch: ok u8[n] (GD_COL_FALSE / TRUE / THROWS / NO_PART) or None."""
        cx = np.ascontiguousarray(np.asarray(ctx, dtype=np.uint32))
        cf, tb = self._opt(ctx_flags, np.uint8), self._opt(turn, np.uint8)
        out = np.zeros(len(cx), np.uint8) if ok else None
        p = lambda a: None if a is None else _ptr(a)
        self._c(lib.gd_collect_touch(self.h, C.byref(st), n_ctx, p(cf), _ptr(cx), p(tb), len(cx), now, p(out)))
        return out

    def collect_idle(self, st: gd_collect_state, n_ctx: int, event, now: int, ok: bool = True):
        ev = np.ascontiguousarray(np.asarray(event, dtype=np.uint8))
        out = np.zeros(n_ctx, np.uint8) if ok else None
        self._c(lib.gd_collect_idle(self.h, C.byref(st), n_ctx, _ptr(ev), now, None if out is None else _ptr(out)))
        return out

    def _collect_scan(self, fn, st, n_ctx, ctx_flags, num_running, wait_offsets, verdict, *mid):
        assert ctx_flags.dtype == np.uint8 and ctx_flags.flags.c_contiguous       # updated in place
        nr, wo = self._opt(num_running, np.uint32), self._opt(wait_offsets, np.uint32)
        out, out_n = np.zeros(max(n_ctx, 1), np.uint32), np.zeros(1, np.uint32)
        vd = np.zeros(n_ctx, np.uint8) if verdict else None
        p = lambda a: None if a is None else _ptr(a)
        self._c(fn(self.h, C.byref(st), n_ctx, _ptr(ctx_flags), p(nr), p(wo), *mid, _ptr(out), _ptr(out_n), p(vd)))
        return out[:int(out_n[0])].copy(), vd

    def collect_scan_stale(self, st: gd_collect_state, n_ctx: int, ctx_flags, num_running, now: int, wait_offsets=None,
                           verdict: bool = True):
        """gd_collect_scan_stale: (condemned u32[out_n] by ticket then context, verdict u8[n_ctx] or None);
        ctx_flags (uint8 array) and the state's arrays are updated in place."""
        return self._collect_scan(lib.gd_collect_scan_stale, st, n_ctx, ctx_flags, num_running, wait_offsets, verdict,
                                  now)

    def collect_scan_all(self, st: gd_collect_state, n_ctx: int, ctx_flags, num_running, now: int, age_limit_ticks: int,
                         wait_offsets=None, verdict: bool = True):
        return self._collect_scan(lib.gd_collect_scan_all, st, n_ctx, ctx_flags, num_running, wait_offsets, verdict,
                                  now, age_limit_ticks)

    def collect_count_recent(self, st: gd_collect_state, n_ctx: int, now: int, shortest_age_limit: int,
                             recency: int) -> int:
        out = np.zeros(1, np.uint64)
        self._c(lib.gd_collect_count_recent(self.h, C.byref(st), n_ctx, now, shortest_age_limit, recency, _ptr(out)))
        return int(out[0])

    # the device forms: st over device addresses, every array a device address (None = NULL), enqueue-only
    def collect_schedule_device(self, st, n_ctx: int, d_ctx, n: int, now: int, d_status=None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_collect_schedule_device(self.h, C.byref(st), n_ctx, V(d_ctx), n, now, V(d_status)))

    def collect_cancel_device(self, st, n_ctx: int, d_ctx, n: int, d_cancelled=None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_collect_cancel_device(self.h, C.byref(st), n_ctx, V(d_ctx), n, V(d_cancelled)))

    def collect_touch_device(self, st, n_ctx: int, d_ctx_flags, d_ctx, d_turn, n: int, now: int, d_ok=None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_collect_touch_device(self.h, C.byref(st), n_ctx, V(d_ctx_flags), V(d_ctx), V(d_turn), n, now,
                                            V(d_ok)))

    def collect_idle_device(self, st, n_ctx: int, d_event, now: int, d_ok=None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_collect_idle_device(self.h, C.byref(st), n_ctx, V(d_event), now, V(d_ok)))

    def collect_scan_stale_device(self, st, n_ctx: int, d_ctx_flags, d_num_running, d_wait_offsets, now: int,
                                  d_out_ctx, d_out_n, d_verdict=None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_collect_scan_stale_device(self.h, C.byref(st), n_ctx, V(d_ctx_flags), V(d_num_running),
                                                 V(d_wait_offsets), now, V(d_out_ctx), V(d_out_n), V(d_verdict)))

    def collect_scan_all_device(self, st, n_ctx: int, d_ctx_flags, d_num_running, d_wait_offsets, now: int,
                                age_limit_ticks: int, d_out_ctx, d_out_n, d_verdict=None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_collect_scan_all_device(self.h, C.byref(st), n_ctx, V(d_ctx_flags), V(d_num_running),
                                               V(d_wait_offsets), now, age_limit_ticks, V(d_out_ctx), V(d_out_n),
                                               V(d_verdict)))

    def collect_count_recent_device(self, st, n_ctx: int, now: int, shortest_age_limit: int, recency: int, d_count):
        self._c(lib.gd_collect_count_recent_device(self.h, C.byref(st), n_ctx, now, shortest_age_limit, recency,
                                                   C.c_void_p(d_count or 0)))

    # -- callback table (InsideRuntimeClient.callbacks) --------------------------------------------
    def callbacks_configure(self, capacity_hint: int, max_resend_count: int = 0, resend_on_timeout: bool = False,
                            period_ticks: int = 0):
        self._c(lib.gd_callbacks_configure(self.h, capacity_hint, max_resend_count, int(resend_on_timeout),
                                           period_ticks))

    def callbacks_clear(self):
        self._c(lib.gd_callbacks_clear(self.h))

    def callbacks_count(self) -> Tuple[int, int]:
        """gd_callbacks_count: (live entries, slots)."""
        live, cap = C.c_uint64(0), C.c_uint64(0)
        self._c(lib.gd_callbacks_count(self.h, C.byref(live), C.byref(cap)))
        return int(live.value), int(cap.value)

    def callbacks_add(self, ids, handles, deadlines) -> np.ndarray:
        """gd_callbacks_add: added u8[n]."""
        i, hd, dl = self._opt(ids, np.int64), self._opt(handles, np.uint32), self._opt(deadlines, np.int64)
        out = np.zeros(len(i), np.uint8)
        self._c(lib.gd_callbacks_add(self.h, _ptr(i), _ptr(hd), _ptr(dl), len(i), _ptr(out)))
        return out

    def callbacks_set_target(self, ids, silo) -> np.ndarray:
        """gd_callbacks_set_target: found u8[n]."""
        i, s = self._opt(ids, np.int64), self._opt(silo, np.uint32)
        out = np.zeros(len(i), np.uint8)
        self._c(lib.gd_callbacks_set_target(self.h, _ptr(i), _ptr(s), len(i), _ptr(out)))
        return out

    def callbacks_lookup(self, ids):
        """gd_callbacks_lookup: (handle u32, resend u32, silo u32, found u8)."""
        i = self._opt(ids, np.int64)
        n = len(i)
        hd, rs, sl, fd = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        self._c(lib.gd_callbacks_lookup(self.h, _ptr(i), n, _ptr(hd), _ptr(rs), _ptr(sl), _ptr(fd)))
        return hd, rs, sl, fd

    def callbacks_respond(self, ids, result=None, rejection_type=None, flags=None, turn=None, fire: bool = True):
        """gd_callbacks_respond: (outcome u8, out_flags u8, handle u32[, fire_idx u32[n_fire]])."""
        i = self._opt(ids, np.int64)
        n = len(i)
        rs, rj = self._opt(result, np.uint8), self._opt(rejection_type, np.uint8)
        fl, tn = self._opt(flags, np.uint8), self._opt(turn, np.uint8)
        p = lambda a: None if a is None else _ptr(a)
        oc, of, hd = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        fi = np.zeros(max(n, 1), np.uint32) if fire else None
        nf = np.zeros(1, np.uint32) if fire else None
        self._c(lib.gd_callbacks_respond(self.h, _ptr(i), p(rs), p(rj), p(fl), p(tn), n, _ptr(oc), _ptr(of), _ptr(hd),
                                         p(fi), p(nf)))
        return (oc, of, hd, fi[:int(nf[0])].copy()) if fire else (oc, of, hd)

    def _callbacks_scan(self, fn, arg, cap: int):
        ids, hd, kd = np.zeros(max(cap, 1), np.int64), np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint8)
        n = np.zeros(1, np.uint32)
        self._c(fn(self.h, arg, cap, _ptr(ids), _ptr(hd), _ptr(kd), _ptr(n)))
        k = int(n[0])
        return ids[:k].copy(), hd[:k].copy(), kd[:k].copy()

    def callbacks_expire(self, now: int, cap: int):
        """gd_callbacks_expire: (id i64, handle u32, kind u8) of the due entries, in no particular order."""
        return self._callbacks_scan(lib.gd_callbacks_expire, now, cap)

    def callbacks_break_silo(self, silo: int, cap: int):
        """gd_callbacks_break_silo: (id i64, handle u32, kind u8) of the entries whose target is `silo`."""
        return self._callbacks_scan(lib.gd_callbacks_break_silo, silo, cap)

    def callbacks_add_device(self, d_ids: int, d_handles: int, d_deadlines: int, n: int, d_out_added: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_callbacks_add_device(self.h, V(d_ids), V(d_handles), V(d_deadlines), n, V(d_out_added)))

    def callbacks_set_target_device(self, d_ids: int, d_silo: int, n: int, d_out_found: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_callbacks_set_target_device(self.h, V(d_ids), V(d_silo), n, V(d_out_found)))

    def callbacks_lookup_device(self, d_ids: int, n: int, d_out_handle: Optional[int] = None,
                                d_out_resend: Optional[int] = None, d_out_silo: Optional[int] = None,
                                d_out_found: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_callbacks_lookup_device(self.h, V(d_ids), n, V(d_out_handle), V(d_out_resend), V(d_out_silo),
                                               V(d_out_found)))

    def callbacks_respond_device(self, d_ids: int, d_result: Optional[int], d_rejection_type: Optional[int],
                                 d_flags: Optional[int], d_turn: Optional[int], n: int, d_out_outcome: int,
                                 d_out_flags: int, d_out_handle: int, d_fire_idx: Optional[int] = None,
                                 d_n_fire: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_callbacks_respond_device(self.h, V(d_ids), V(d_result), V(d_rejection_type), V(d_flags), V(d_turn),
                                                n, V(d_out_outcome), V(d_out_flags), V(d_out_handle), V(d_fire_idx),
                                                V(d_n_fire)))

    def callbacks_expire_device(self, now: int, cap: int, d_out_id: int, d_out_handle: int, d_out_kind: int, d_n_out: int):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_callbacks_expire_device(self.h, now, cap, V(d_out_id), V(d_out_handle), V(d_out_kind), V(d_n_out)))

    def callbacks_break_silo_device(self, silo: int, cap: int, d_out_id: int, d_out_handle: int, d_out_kind: int,
                                    d_n_out: int):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_callbacks_break_silo_device(self.h, silo, cap, V(d_out_id), V(d_out_handle), V(d_out_kind),
                                                   V(d_n_out)))

    # -- gateway (Messaging/Gateway.cs, GatewayAcceptor.cs) ------------------------------------------
    def gateway_configure(self, n_senders: int, client_drop_timeout: int, route_expiry: int, capacity_hint: int = 0):
        self._c(lib.gd_gateway_configure(self.h, n_senders, client_drop_timeout, route_expiry, capacity_hint))
        self.gateway_n_senders = n_senders

    def gateway_clear(self):
        self._c(lib.gd_gateway_clear(self.h))

    def gateway_count(self) -> Tuple[int, int, int, int]:
        """gd_gateway_count: (live clients, live routes, client slots, route slots)."""
        v = [C.c_uint64(0) for _ in range(4)]
        self._c(lib.gd_gateway_count(self.h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def gateway_open(self, ids, handles):
        """gd_gateway_open: (handle u32, sender u32, new u8, pending u32)."""
        k, hd = keys_array(ids), np.ascontiguousarray(np.asarray(handles, dtype=np.uint32))
        n = len(k)
        oh, os_, on, op = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        self._c(lib.gd_gateway_open(self.h, _ptr(k), _ptr(hd), n, _ptr(oh), _ptr(os_), _ptr(on), _ptr(op)))
        return oh, os_, on, op

    def gateway_close(self, ids, now: int, pending_left=None) -> np.ndarray:
        """gd_gateway_close: found u8[n]."""
        k, pl = keys_array(ids), self._opt(pending_left, np.uint32)
        out = np.zeros(len(k), np.uint8)
        self._c(lib.gd_gateway_close(self.h, _ptr(k), None if pl is None else _ptr(pl), len(k), now, _ptr(out)))
        return out

    def gateway_drop(self, now: int, cap: int):
        """gd_gateway_drop: (id u64[k, 3], handle u32, pending u32) of the dropped clients, in no particular order."""
        ids, hd, pd = np.zeros((max(cap, 1), 3), np.uint64), np.zeros(max(cap, 1), np.uint32), np.zeros(max(cap, 1), np.uint32)
        n = np.zeros(1, np.uint32)
        self._c(lib.gd_gateway_drop(self.h, now, cap, _ptr(ids), _ptr(hd), _ptr(pd), _ptr(n)))
        k = int(n[0])
        return ids[:k].copy(), hd[:k].copy(), pd[:k].copy()

    def gateway_routes_expire(self, now: int) -> int:
        n = np.zeros(1, np.uint32)
        self._c(lib.gd_gateway_routes_expire(self.h, now, _ptr(n)))
        return int(n[0])

    def gateway_lookup(self, ids):
        """gd_gateway_lookup: (handle u32, sender u32, connected u8, since i64, pending u32, found u8, route_silo u32,
        route_time i64, route_found u8)."""
        k = keys_array(ids)
        n = len(k)
        out = [np.zeros(n, t) for t in (np.uint32, np.uint32, np.uint8, np.int64, np.uint32, np.uint8, np.uint32,
                                        np.int64, np.uint8)]
        self._c(lib.gd_gateway_lookup(self.h, _ptr(k), n, *[_ptr(a) for a in out]))
        return tuple(out)

    def gateway_deliver(self, target_grain, sending_grain, sending_silo, now: int, ttl=None, bucket: bool = True):
        """gd_gateway_deliver: (status u8, handle u32, sender u32[, perm, offsets[n_senders + 2]])."""
        t = keys_array(target_grain)
        n = len(t)
        s = None if sending_grain is None else keys_array(sending_grain)
        ss, tl = self._opt(sending_silo, np.uint32), self._opt(ttl, np.int64)
        p = lambda a: None if a is None else _ptr(a)
        st, hd, sd = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        perm = np.zeros(n, np.uint32) if bucket else None
        off = np.zeros(self.gateway_n_senders + 2, np.uint32) if bucket else None
        self._c(lib.gd_gateway_deliver(self.h, _ptr(t), p(s), p(ss), p(tl), n, now, _ptr(st), _ptr(hd), _ptr(sd), p(perm),
                                       p(off)))
        return (st, hd, sd, perm, off) if bucket else (st, hd, sd)

    def gateway_send_queues(self, target_grain, sending_grain, sending_silo, silo, now: int, route_status=None,
                            category=None, ttl=None, bucket: bool = True):
        """gd_gateway_send_queues: (send_status u8, queue u32, handle u32[, perm, offsets[n_queues + n_senders + 5]])."""
        t = keys_array(target_grain)
        n = len(t)
        s = None if sending_grain is None else keys_array(sending_grain)
        ss, sl = self._opt(sending_silo, np.uint32), np.ascontiguousarray(np.asarray(silo, dtype=np.uint32))
        rs, cat, tl = self._opt(route_status, np.uint8), self._opt(category, np.uint8), self._opt(ttl, np.int64)
        p = lambda a: None if a is None else _ptr(a)
        st, q, hd = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        perm = np.zeros(n, np.uint32) if bucket else None
        off = np.zeros(self.send_n_queues + self.gateway_n_senders + 5, np.uint32) if bucket else None
        self._c(lib.gd_gateway_send_queues(self.h, _ptr(t), p(s), p(ss), _ptr(sl), p(rs), p(cat), p(tl), n, now, _ptr(st),
                                           _ptr(q), _ptr(hd), p(perm), p(off)))
        return (st, q, hd, perm, off) if bucket else (st, q, hd)

    def gateway_ingress(self, target_grain, sending_grain, direction=None, ttl=None, overloaded: bool = False,
                        routes: bool = True):
        """gd_gateway_ingress: (status u8, silo u32[, route_idx u32[n_route], route_keys u64[n_route, 3]])."""
        t = keys_array(target_grain)
        n = len(t)
        s = None if sending_grain is None else keys_array(sending_grain)
        d, tl = self._opt(direction, np.uint8), self._opt(ttl, np.int64)
        p = lambda a: None if a is None else _ptr(a)
        st, sl = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
        ri = np.zeros(max(n, 1), np.uint32) if routes else None
        nr = np.zeros(1, np.uint32) if routes else None
        rk = np.zeros((max(n, 1), 3), np.uint64) if routes else None
        self._c(lib.gd_gateway_ingress(self.h, _ptr(t), p(s), p(d), p(tl), n, int(overloaded), _ptr(st), _ptr(sl), p(ri),
                                       p(nr), p(rk)))
        return (st, sl, ri[:int(nr[0])].copy(), rk[:int(nr[0])].copy()) if routes else (st, sl)

    def gateway_open_device(self, d_ids: int, d_handles: int, n: int, d_out_handle: Optional[int] = None,
                            d_out_sender: Optional[int] = None, d_out_new: Optional[int] = None,
                            d_out_pending: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_gateway_open_device(self.h, V(d_ids), V(d_handles), n, V(d_out_handle), V(d_out_sender),
                                           V(d_out_new), V(d_out_pending)))

    def gateway_close_device(self, d_ids: int, d_pending_left: Optional[int], n: int, now: int,
                             d_out_found: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_gateway_close_device(self.h, V(d_ids), V(d_pending_left), n, now, V(d_out_found)))

    def gateway_drop_device(self, now: int, cap: int, d_out_id: int, d_out_handle: int, d_out_pending: int, d_n_out: int):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_gateway_drop_device(self.h, now, cap, V(d_out_id), V(d_out_handle), V(d_out_pending), V(d_n_out)))

    def gateway_routes_expire_device(self, now: int, d_n_removed: int):
        self._c(lib.gd_gateway_routes_expire_device(self.h, now, C.c_void_p(d_n_removed or 0)))

    def gateway_lookup_device(self, d_ids: int, n: int, d_out_handle: Optional[int] = None,
                              d_out_sender: Optional[int] = None, d_out_connected: Optional[int] = None,
                              d_out_since: Optional[int] = None, d_out_pending: Optional[int] = None,
                              d_out_found: Optional[int] = None, d_out_route_silo: Optional[int] = None,
                              d_out_route_time: Optional[int] = None, d_out_route_found: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_gateway_lookup_device(self.h, V(d_ids), n, V(d_out_handle), V(d_out_sender), V(d_out_connected),
                                             V(d_out_since), V(d_out_pending), V(d_out_found), V(d_out_route_silo),
                                             V(d_out_route_time), V(d_out_route_found)))

    def gateway_deliver_device(self, d_target_grain: int, d_sending_grain: Optional[int], d_sending_silo: Optional[int],
                               d_ttl: Optional[int], n: int, now: int, d_out_status: int,
                               d_out_handle: Optional[int] = None, d_out_sender: Optional[int] = None,
                               d_perm: Optional[int] = None, d_offsets: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_gateway_deliver_device(self.h, V(d_target_grain), V(d_sending_grain), V(d_sending_silo), V(d_ttl), n,
                                              now, V(d_out_status), V(d_out_handle), V(d_out_sender), V(d_perm),
                                              V(d_offsets)))

    def gateway_send_queues_device(self, d_target_grain: int, d_sending_grain: Optional[int],
                                   d_sending_silo: Optional[int], d_silo: int, d_route_status: Optional[int],
                                   d_category: Optional[int], d_ttl: Optional[int], n: int, now: int, d_send_status: int,
                                   d_queue: Optional[int] = None, d_out_handle: Optional[int] = None,
                                   d_perm: Optional[int] = None, d_offsets: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_gateway_send_queues_device(self.h, V(d_target_grain), V(d_sending_grain), V(d_sending_silo),
                                                  V(d_silo), V(d_route_status), V(d_category), V(d_ttl), n, now,
                                                  V(d_send_status), V(d_queue), V(d_out_handle), V(d_perm), V(d_offsets)))

    def gateway_ingress_device(self, d_target_grain: int, d_sending_grain: Optional[int], d_direction: Optional[int],
                               d_ttl: Optional[int], n: int, overloaded: bool, d_out_status: int,
                               d_out_silo: Optional[int] = None, d_route_idx: Optional[int] = None,
                               d_n_route: Optional[int] = None, d_route_keys: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_gateway_ingress_device(self.h, V(d_target_grain), V(d_sending_grain), V(d_direction), V(d_ttl), n,
                                              int(overloaded), V(d_out_status), V(d_out_silo), V(d_route_idx),
                                              V(d_n_route), V(d_route_keys)))

    # -- stateless workers (Placement/StatelessWorkerDirector.cs, Catalog/ActivationDirectory.cs) ----------
    def workers_configure(self, capacity: int, slot_capacity: int, default_max_local: int):
        """gd_workers_configure: sets expected, list entries a set, MaxLocal of a message that brings none."""
        self._c(lib.gd_workers_configure(self.h, capacity, slot_capacity, default_max_local))
        self.workers_slot_capacity = slot_capacity

    def workers_clear(self):
        self._c(lib.gd_workers_clear(self.h))

    def workers_count(self) -> Tuple[int, int]:
        """gd_workers_count: (live sets, table slots)."""
        v = [C.c_uint64(0) for _ in range(2)]
        self._c(lib.gd_workers_count(self.h, *[C.byref(x) for x in v]))
        return tuple(int(x.value) for x in v)

    def workers_add(self, grains, ctx, max_local=None) -> np.ndarray:
        """gd_workers_add: status u8[n] (WK_ADDED / WK_FULL / WK_NOT_GRAIN)."""
        k, c = keys_array(grains), np.ascontiguousarray(np.asarray(ctx, dtype=np.uint32))
        ml = self._opt(max_local, np.int32)
        st = np.zeros(len(k), np.uint8)
        self._c(lib.gd_workers_add(self.h, _ptr(k), _ptr(c), None if ml is None else _ptr(ml), len(k), _ptr(st)))
        return st

    def workers_remove(self, grains, ctx) -> np.ndarray:
        """gd_workers_remove: removed u8[n]."""
        k, c = keys_array(grains), np.ascontiguousarray(np.asarray(ctx, dtype=np.uint32))
        out = np.zeros(len(k), np.uint8)
        self._c(lib.gd_workers_remove(self.h, _ptr(k), _ptr(c), len(k), _ptr(out)))
        return out

    def workers_lookup(self, grains):
        """gd_workers_lookup: (count u32[n], max_local u32[n], list u32[n, slot_capacity], unused tail 0xFFFFFFFF)."""
        k = keys_array(grains)
        n = len(k)
        cnt, ml = np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        lst = np.zeros((n, self.workers_slot_capacity), np.uint32)
        self._c(lib.gd_workers_lookup(self.h, _ptr(k), n, _ptr(cnt), _ptr(ml), _ptr(lst)))
        return cnt, ml, lst

    def workers_select(self, grains, ctx_base: int, ctx_flags, num_running, wait_offsets=None, max_local=None,
                       draw=None, new_list: bool = True):
        """gd_workers_select: (ctx u32[n], pick u8[n], new_idx u32[n_new]) -- without new_list (ctx, pick)."""
        k = keys_array(grains)
        n = len(k)
        cf, nr = self._opt(ctx_flags, np.uint8), self._opt(num_running, np.uint32)
        wo, ml, dr = self._opt(wait_offsets, np.uint32), self._opt(max_local, np.int32), self._opt(draw, np.uint32)
        n_ctx = 0 if cf is None else len(cf)
        p = lambda a: None if a is None or a.size == 0 else _ptr(a)
        ctx, pick = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        ni = np.zeros(max(n, 1), np.uint32) if new_list else None
        nn = np.zeros(1, np.uint32) if new_list else None
        self._c(lib.gd_workers_select(self.h, _ptr(k), n, p(ml), p(dr), ctx_base, n_ctx, p(cf), p(nr), p(wo), _ptr(ctx),
                                      _ptr(pick), p(ni), p(nn)))
        return (ctx, pick, ni[:int(nn[0])].copy()) if new_list else (ctx, pick)

    def workers_add_device(self, d_grains: int, d_ctx: int, d_max_local: Optional[int], n: int, d_out_status: int):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_workers_add_device(self.h, V(d_grains), V(d_ctx), V(d_max_local), n, V(d_out_status)))

    def workers_remove_device(self, d_grains: int, d_ctx: int, n: int, d_out_removed: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_workers_remove_device(self.h, V(d_grains), V(d_ctx), n, V(d_out_removed)))

    def workers_lookup_device(self, d_grains: int, n: int, d_out_count: Optional[int] = None,
                              d_out_max_local: Optional[int] = None, d_out_list: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_workers_lookup_device(self.h, V(d_grains), n, V(d_out_count), V(d_out_max_local), V(d_out_list)))

    def workers_select_device(self, d_grains: int, n: int, d_max_local: Optional[int], d_draw: Optional[int],
                              ctx_base: int, n_ctx: int, d_ctx_flags: Optional[int], d_num_running: Optional[int],
                              d_wait_offsets: Optional[int], d_ctx: int, d_pick: int, d_new_idx: Optional[int] = None,
                              d_n_new: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_workers_select_device(self.h, V(d_grains), n, V(d_max_local), V(d_draw), ctx_base, n_ctx,
                                             V(d_ctx_flags), V(d_num_running), V(d_wait_offsets), V(d_ctx), V(d_pick),
                                             V(d_new_idx), V(d_n_new)))

    def upsert(self, keys, acts, silos) -> np.ndarray:
        """gd_dir_upsert: overwrite, the last item of a grain wins; acts may hold GD_ACT_MULTI."""
        k = keys_array(keys)
        n = len(k)
        vals = np.zeros((n, 2), dtype=np.uint32)
        vals[:, 0] = acts
        vals[:, 1] = silos
        ins = np.zeros(n, dtype=np.uint8)
        self._c(lib.gd_dir_upsert(self.h, _ptr(k), _ptr(vals), n, _ptr(ins)))
        return ins

    def unregister(self, keys, acts) -> np.ndarray:
        k = keys_array(keys)
        a = np.ascontiguousarray(np.asarray(acts, dtype=np.uint32))
        out = np.zeros(len(k), dtype=np.uint8)
        self._c(lib.gd_dir_unregister(self.h, _ptr(k), _ptr(a), len(k), _ptr(out)))
        return out

    def lookup(self, keys):
        k = keys_array(keys)
        n = len(k)
        out = np.zeros((n, 2), dtype=np.uint32)
        found = np.zeros(n, dtype=np.uint8)
        self._c(lib.gd_dir_lookup(self.h, _ptr(k), n, _ptr(out), _ptr(found)))
        return out[:, 0].copy(), out[:, 1].copy(), found

    def clear(self):
        self._c(lib.gd_dir_clear(self.h))

    def split(self, keep_silos, move: bool = True):
        """GrainDirectoryPartition.Split by "owner under the installed ring is not kept here"
        (SURVEY 8 f4).  keep_silos: iterable of silo indices this handle keeps.  Returns
        (keys (n,3) u64, acts u32, silos u32) in slot order; move=True removes them here."""
        ks = [int(x) for x in keep_silos]
        keep = np.zeros(max(ks) + 1 if ks else 1, dtype=np.uint8)
        keep[ks] = 1
        n = C.c_uint64(0)
        self._c(lib.gd_dir_split(self.h, _ptr(keep), len(keep), 1 if move else 0, None, None, 0, C.byref(n)))
        keys = np.zeros((n.value, 3), dtype=np.uint64)
        vals = np.zeros((n.value, 2), dtype=np.uint32)
        if n.value:
            got = C.c_uint64(0)
            self._c(lib.gd_dir_split(self.h, _ptr(keep), len(keep), 1 if move else 0, _ptr(keys), _ptr(vals),
                                     n.value, C.byref(got)))
            assert got.value == n.value
        return keys, vals[:, 0].copy(), vals[:, 1].copy()

    @staticmethod
    def keep_mask(keep_silos, n_silos: int) -> np.ndarray:
        keep = np.zeros(max(n_silos, 1), dtype=np.uint8)
        keep[[int(x) for x in keep_silos]] = 1
        return keep

    def split_device(self, keep: np.ndarray, move: bool, d_keys: Optional[int], d_vals: Optional[int],
                     capacity: int) -> int:
        """gd_dir_split_device; d_keys None = size query.  Returns the entries selected."""
        keep = np.ascontiguousarray(keep, dtype=np.uint8)
        n = C.c_uint64(0)
        self._c(lib.gd_dir_split_device(self.h, _ptr(keep), len(keep), 1 if move else 0,
                                        C.c_void_p(d_keys) if d_keys else None,
                                        C.c_void_p(d_vals) if d_vals else None, capacity, C.byref(n)))
        return n.value

    def rehash(self, capacity: int):
        self._c(lib.gd_dir_rehash(self.h, capacity))

    # -- hot path (host arrays) --------------------------------------------------
    def route(self, keys):
        k = keys_array(keys)
        n = len(k)
        silo = np.zeros(n, dtype=np.uint32)
        act = np.zeros(n, dtype=np.uint32)
        st = np.zeros(n, dtype=np.uint8)
        self._c(lib.gd_route(self.h, _ptr(k), n, _ptr(silo), _ptr(act), _ptr(st)))
        return st, silo, act

    def bucket(self, acts, n_act: int):
        a = np.ascontiguousarray(np.asarray(acts, dtype=np.uint32))
        perm = np.zeros(len(a), dtype=np.uint32)
        off = np.zeros(n_act + 2, dtype=np.uint32)
        self._c(lib.gd_bucket(self.h, _ptr(a), len(a), n_act, _ptr(perm), _ptr(off)))
        return perm, off

    def route_bucket(self, keys, n_act: int):
        k = keys_array(keys)
        n = len(k)
        silo = np.zeros(n, dtype=np.uint32)
        act = np.zeros(n, dtype=np.uint32)
        st = np.zeros(n, dtype=np.uint8)
        perm = np.zeros(n, dtype=np.uint32)
        off = np.zeros(n_act + 2, dtype=np.uint32)
        self._c(lib.gd_route_bucket(self.h, _ptr(k), n, n_act, _ptr(silo), _ptr(act), _ptr(st), _ptr(perm), _ptr(off)))
        return st, silo, act, perm, off

    # -- compact route: (class, N1) records in, packed routes out -----------
    def classes_set(self, type_code_data):
        """gd_classes_set: the class table; class id = index.  An empty list clears it."""
        t = np.ascontiguousarray(np.asarray(type_code_data, dtype=np.uint64))
        self._c(lib.gd_classes_set(self.h, _ptr(t) if len(t) else None, len(t)))

    def classes_get(self) -> np.ndarray:
        out = np.zeros(256, dtype=np.uint64)
        n = C.c_uint32(0)
        self._c(lib.gd_classes_get(self.h, _ptr(out), 256, C.byref(n)))
        return out[: n.value].copy()

    @staticmethod
    def _records(cls, n1, n1_width):
        """(cls u8[n] or None, n1 u32[n] / u64[n], width): n1_width None takes the width of n1's dtype (4 for a
        4-byte integer array, else 8)."""
        a = np.asarray(n1)
        w = n1_width or (4 if a.dtype.kind in "iu" and a.dtype.itemsize == 4 else 8)
        a = np.ascontiguousarray(a, dtype=np.uint32 if w == 4 else np.uint64)
        c = None if cls is None else np.ascontiguousarray(np.asarray(cls, dtype=np.uint8))
        assert c is None or len(c) == len(a), "one class id per N1"
        return c, a, w

    def route_compact(self, cls, n1, n1_width: Optional[int] = None):
        """gd_route_compact: (status u8[n], silo16 u16[n], act u32[n]) of the keys {0, n1[i], classes[cls[i]]};
        cls None: every message is class 0."""
        c, a, w = self._records(cls, n1, n1_width)
        n = len(a)
        act = np.zeros(n, dtype=np.uint32)
        silo = np.zeros(n, dtype=np.uint16)
        st = np.zeros(n, dtype=np.uint8)
        self._c(lib.gd_route_compact(self.h, None if c is None else _ptr(c), _ptr(a), w, n, _ptr(act), _ptr(silo),
                                     _ptr(st)))
        return st, silo, act

    def route_bucket_compact(self, cls, n1, n_act: int, n1_width: Optional[int] = None):
        """gd_route_bucket_compact: (status, silo16, act, perm u32[n], offsets u32[n_act + 2])."""
        c, a, w = self._records(cls, n1, n1_width)
        n = len(a)
        act = np.zeros(n, dtype=np.uint32)
        silo = np.zeros(n, dtype=np.uint16)
        st = np.zeros(n, dtype=np.uint8)
        perm = np.zeros(n, dtype=np.uint32)
        off = np.zeros(n_act + 2, dtype=np.uint32)
        self._c(lib.gd_route_bucket_compact(self.h, None if c is None else _ptr(c), _ptr(a), w, n, n_act, _ptr(act),
                                            _ptr(silo), _ptr(st), _ptr(perm), _ptr(off)))
        return st, silo, act, perm, off

    def route_compact_device(self, d_cls: Optional[int], d_n1: int, n1_width: int, n: int, d_act: int, d_silo16: int,
                             d_status: int, d_wide: Optional[int] = None):
        """gd_route_compact_device: device pointers, enqueue only; d_wide (optional) gets the count of silos that
        do not fit 16 bits."""
        V = C.c_void_p
        self._c(lib.gd_route_compact_device(self.h, V(d_cls), V(d_n1), n1_width, n, V(d_act), V(d_silo16), V(d_status),
                                            V(d_wide)))

    def route_bucket_compact_device(self, d_cls: Optional[int], d_n1: int, n1_width: int, n: int, n_act: int,
                                    d_act: int, d_silo16: int, d_status: int, d_perm: int, d_offsets: int,
                                    d_wide: Optional[int] = None):
        V = C.c_void_p
        self._c(lib.gd_route_bucket_compact_device(self.h, V(d_cls), V(d_n1), n1_width, n, n_act, V(d_act), V(d_silo16),
                                                   V(d_status), V(d_perm), V(d_offsets), V(d_wide)))

    # -- KeyExt grains (string keys, compound keys, geo clients) ------------------------
    @staticmethod
    def _ext(exts, n: int) -> KeyExtBatch:
        x = exts if isinstance(exts, KeyExtBatch) else KeyExtBatch(list(exts))
        assert len(x.length) == n, "one KeyExt entry per key"
        return x

    def register_ext(self, keys, exts, acts, silos):
        k = keys_array(keys)
        n = len(k)
        x = self._ext(exts, n)
        vals = np.zeros((n, 2), dtype=np.uint32)
        vals[:, 0] = acts
        vals[:, 1] = silos
        out = np.zeros((n, 2), dtype=np.uint32)
        ins = np.zeros(n, dtype=np.uint8)
        self._c(lib.gd_dir_register_ext(self.h, _ptr(k), C.byref(x.struct), _ptr(vals), n, _ptr(out), _ptr(ins)))
        return out[:, 0].copy(), out[:, 1].copy(), ins

    def unregister_ext(self, keys, exts, acts) -> np.ndarray:
        k = keys_array(keys)
        n = len(k)
        x = self._ext(exts, n)
        a = np.ascontiguousarray(acts, dtype=np.uint32)
        out = np.zeros(n, dtype=np.uint8)
        self._c(lib.gd_dir_unregister_ext(self.h, _ptr(k), C.byref(x.struct), _ptr(a), n, _ptr(out)))
        return out

    def lookup_ext(self, keys, exts):
        k = keys_array(keys)
        n = len(k)
        x = self._ext(exts, n)
        vals = np.zeros((n, 2), dtype=np.uint32)
        found = np.zeros(n, dtype=np.uint8)
        self._c(lib.gd_dir_lookup_ext(self.h, _ptr(k), C.byref(x.struct), n, _ptr(vals), _ptr(found)))
        return found, vals[:, 0].copy(), vals[:, 1].copy()

    def uniform_hashes_ext(self, keys, exts) -> np.ndarray:
        k = keys_array(keys)
        n = len(k)
        x = self._ext(exts, n)
        out = np.zeros(n, dtype=np.uint32)
        self._c(lib.gd_uniform_hashes_ext(self.h, _ptr(k), C.byref(x.struct), n, _ptr(out)))
        return out

    def ext_stats(self) -> dict:
        live, cap, heap = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._c(lib.gd_dir_ext_stats(self.h, C.byref(live), C.byref(cap), C.byref(heap)))
        return {"live": live.value, "capacity": cap.value, "heap_bytes": heap.value}

    def route_ext(self, keys, exts):
        k = keys_array(keys)
        n = len(k)
        x = self._ext(exts, n)
        silo = np.zeros(n, dtype=np.uint32)
        act = np.zeros(n, dtype=np.uint32)
        st = np.zeros(n, dtype=np.uint8)
        self._c(lib.gd_route_ext(self.h, _ptr(k), C.byref(x.struct), n, _ptr(silo), _ptr(act), _ptr(st)))
        return st, silo, act

    def route_bucket_ext(self, keys, exts, n_act: int):
        k = keys_array(keys)
        n = len(k)
        x = self._ext(exts, n)
        silo = np.zeros(n, dtype=np.uint32)
        act = np.zeros(n, dtype=np.uint32)
        st = np.zeros(n, dtype=np.uint8)
        perm = np.zeros(n, dtype=np.uint32)
        off = np.zeros(n_act + 2, dtype=np.uint32)
        self._c(lib.gd_route_bucket_ext(self.h, _ptr(k), C.byref(x.struct), n, n_act, _ptr(silo), _ptr(act), _ptr(st),
                                        _ptr(perm), _ptr(off)))
        return st, silo, act, perm, off

    def route_bucket_ext_device(self, d_keys: int, d_bytes: int, d_offset: int, d_length: int, bytes_len: int, n: int,
                                n_act: int, d_silo: int, d_act: int, d_status: int, d_perm: int, d_offsets: int):
        dx = gd_key_ext(d_bytes, d_offset, d_length, bytes_len)
        self._c(lib.gd_route_bucket_ext_device(self.h, C.c_void_p(d_keys), C.byref(dx), n, n_act, C.c_void_p(d_silo),
                                               C.c_void_p(d_act), C.c_void_p(d_status), C.c_void_p(d_perm),
                                               C.c_void_p(d_offsets)))

    # -- non-owner directory cache -------------------------------------
    @staticmethod
    def _silo_mask(silos, n_silos: int, default: int) -> np.ndarray:
        m = np.full(max(n_silos, 1), default, dtype=np.uint8)
        if silos is not None:
            m[:] = 0
            m[[int(x) for x in silos]] = 1
        return m

    def cache_configure(self, max_size: int, local_silos, n_silos: int, valid_silos=None):
        """LocalLookup mode: grains owned by `local_silos` are probed here, the rest in an
        LRU cache of `max_size` entries (valid_silos None = every silo valid)."""
        loc = self._silo_mask(local_silos, n_silos, 0)
        val = self._silo_mask(valid_silos, n_silos, 1)
        self._c(lib.gd_cache_configure(self.h, max_size, _ptr(loc), _ptr(val), n_silos))

    def cache_set_silos(self, local_silos, n_silos: int, valid_silos=None):
        loc = self._silo_mask(local_silos, n_silos, 0)
        val = self._silo_mask(valid_silos, n_silos, 1)
        self._c(lib.gd_cache_set_silos(self.h, _ptr(loc), _ptr(val), n_silos))

    def cache_add(self, keys, acts, silos, versions, exts=None):
        """AddOrUpdate in order; exts (one per key, see KeyExtBatch) keys KeyExt grains by their string."""
        k = keys_array(keys)
        n = len(k)
        vals = np.zeros((n, 2), dtype=np.uint32)
        vals[:, 0] = acts
        vals[:, 1] = silos
        ver = np.ascontiguousarray(np.asarray(versions, dtype=np.int32))
        if exts is None:
            self._c(lib.gd_cache_add(self.h, _ptr(k), _ptr(vals), _ptr(ver), n))
        else:
            x = self._ext(exts, n)
            self._c(lib.gd_cache_add_ext(self.h, _ptr(k), C.byref(x.struct), _ptr(vals), _ptr(ver), n))

    def cache_remove(self, keys, exts=None) -> np.ndarray:
        k = keys_array(keys)
        out = np.zeros(len(k), dtype=np.uint8)
        if exts is None:
            self._c(lib.gd_cache_remove(self.h, _ptr(k), len(k), _ptr(out)))
        else:
            x = self._ext(exts, len(k))
            self._c(lib.gd_cache_remove_ext(self.h, _ptr(k), C.byref(x.struct), len(k), _ptr(out)))
        return out

    def cache_lookup(self, keys, exts=None):
        """Returns (found u8, act u32, silo u32, version i32)."""
        k = keys_array(keys)
        n = len(k)
        vals = np.zeros((n, 2), dtype=np.uint32)
        ver = np.zeros(n, dtype=np.int32)
        found = np.zeros(n, dtype=np.uint8)
        if exts is None:
            self._c(lib.gd_cache_lookup(self.h, _ptr(k), n, _ptr(vals), _ptr(ver), _ptr(found)))
        else:
            x = self._ext(exts, n)
            self._c(lib.gd_cache_lookup_ext(self.h, _ptr(k), C.byref(x.struct), n, _ptr(vals), _ptr(ver),
                                            _ptr(found)))
        return found, vals[:, 0].copy(), vals[:, 1].copy(), ver

    def cache_clear(self):
        self._c(lib.gd_cache_clear(self.h))

    def cache_stats(self) -> dict:
        s = gd_cache_stats()
        self._c(lib.gd_cache_stats_get(self.h, C.byref(s)))
        return {name: int(getattr(s, name)) for name, _ in gd_cache_stats._fields_}

    def cache_entries(self) -> dict:
        """key tuple -> (act, silo, version, generation)."""
        n = C.c_uint64(0)
        self._c(lib.gd_cache_entries(self.h, None, None, None, None, 0, C.byref(n)))
        m = n.value
        k = np.zeros((max(m, 1), 3), dtype=np.uint64)
        v = np.zeros((max(m, 1), 2), dtype=np.uint32)
        ver = np.zeros(max(m, 1), dtype=np.int32)
        gen = np.zeros(max(m, 1), dtype=np.uint64)
        if m:
            self._c(lib.gd_cache_entries(self.h, _ptr(k), _ptr(v), _ptr(ver), _ptr(gen), m, C.byref(n)))
        return {tuple(int(x) for x in k[i]): (int(v[i, 0]), int(v[i, 1]), int(ver[i]), int(gen[i]))
                for i in range(m)}

    def cache_entries_ext(self) -> dict:
        """(n0, n1, tcd) or (n0, n1, tcd, KeyExt bytes) -> (act, silo, version, generation)."""
        n, nb = C.c_uint64(0), C.c_uint64(0)
        self._c(lib.gd_cache_entries_ext(self.h, None, None, None, None, None, None, None, 0, 0, C.byref(n),
                                         C.byref(nb)))
        m, b = n.value, nb.value
        k = np.zeros((max(m, 1), 3), dtype=np.uint64)
        v = np.zeros((max(m, 1), 2), dtype=np.uint32)
        ver = np.zeros(max(m, 1), dtype=np.int32)
        gen = np.zeros(max(m, 1), dtype=np.uint64)
        xl = np.zeros(max(m, 1), dtype=np.int32)
        xo = np.zeros(max(m, 1), dtype=np.uint64)
        blob = np.zeros(max(b, 1), dtype=np.uint8)
        if m:
            self._c(lib.gd_cache_entries_ext(self.h, _ptr(k), _ptr(v), _ptr(ver), _ptr(gen), _ptr(xl), _ptr(xo),
                                             _ptr(blob), m, b, C.byref(n), C.byref(nb)))
        out = {}
        for i in range(m):
            key = tuple(int(x) for x in k[i])
            if xl[i] >= 0:
                key = key + (bytes(blob[int(xo[i]):int(xo[i]) + int(xl[i])]),)
            out[key] = (int(v[i, 0]), int(v[i, 1]), int(ver[i]), int(gen[i]))
        return out

    # -- the directory cache's maintainer ------------------------------
    def cache_maintain_configure(self, initial_ticks: int, max_ticks: int, growth: float, now: int):
        self._c(lib.gd_cache_maintain_configure(self.h, initial_ticks, max_ticks, growth, now))

    def cache_clock_set(self, now: int):
        self._c(lib.gd_cache_clock_set(self.h, now))

    def cache_entries_age(self):
        """(refreshed i64, timer i64, num_accesses i32) in the slot order of cache_entries()."""
        n = C.c_uint64(0)
        self._c(lib.gd_cache_entries_age(self.h, None, None, None, 0, C.byref(n)))
        m = n.value
        r = np.zeros(max(m, 1), dtype=np.int64)
        t = np.zeros(max(m, 1), dtype=np.int64)
        a = np.zeros(max(m, 1), dtype=np.int32)
        if m:
            self._c(lib.gd_cache_entries_age(self.h, _ptr(r), _ptr(t), _ptr(a), m, C.byref(n)))
        return r[:m], t[:m], a[:m]

    def cache_scan(self, now: int):
        """AdaptiveDirectoryCacheMaintainer.Run's loop at `now`.  Returns (counts, lists): counts the five
        numbers (seen, self-owned, fresh, dropped, to refresh); lists an insertion-ordered dict owner silo ->
        (keys u64[m, 3], etags i32[m], exts: list of bytes or None per key), with lists.slots the cache slots."""
        counts = np.zeros(5, dtype=np.uint64)
        no, n, nb = C.c_uint32(0), C.c_uint32(0), C.c_uint64(0)
        self._c(lib.gd_cache_scan(self.h, now, _ptr(counts), C.byref(no), C.byref(n), C.byref(nb)))
        no, n, nb = no.value, n.value, nb.value
        owner = np.zeros(max(no, 1), dtype=np.uint32)
        offs = np.zeros(no + 1, dtype=np.uint32)
        keys = np.zeros((max(n, 1), 3), dtype=np.uint64)
        etags = np.zeros(max(n, 1), dtype=np.int32)
        slots = np.zeros(max(n, 1), dtype=np.uint32)
        xl = np.zeros(max(n, 1), dtype=np.int32)
        xo = np.zeros(max(n, 1), dtype=np.uint64)
        blob = np.zeros(max(nb, 1), dtype=np.uint8)
        self._c(lib.gd_cache_scan_fetch(self.h, _ptr(owner), _ptr(offs), _ptr(keys), _ptr(etags), _ptr(slots), _ptr(xl),
                                        _ptr(xo), _ptr(blob), no, n, nb))
        lists = ScanLists()
        lists.slots, lists.offsets, lists.owners = slots[:n].copy(), offs.copy(), owner[:no].copy()
        for r in range(no):
            a, b = int(offs[r]), int(offs[r + 1])
            exts = [bytes(blob[int(xo[k]):int(xo[k]) + int(xl[k])]) if xl[k] >= 0 else None for k in range(a, b)]
            lists[int(owner[r])] = (keys[a:b].copy(), etags[a:b].copy(), exts)
        return [int(x) for x in counts], lists

    def dir_lookup_many(self, keys, etags):
        """LookUpMany: (kind u8, act u32, silo u32, tag i32) per item."""
        k = keys_array(keys)
        n = len(k)
        e = np.ascontiguousarray(np.asarray(etags, dtype=np.int32))
        kind = np.zeros(max(n, 1), dtype=np.uint8)
        vals = np.zeros((max(n, 1), 2), dtype=np.uint32)
        tags = np.zeros(max(n, 1), dtype=np.int32)
        self._c(lib.gd_dir_lookup_many(self.h, _ptr(k), _ptr(e), n, _ptr(kind), _ptr(vals), _ptr(tags)))
        return kind[:n], vals[:n, 0].copy(), vals[:n, 1].copy(), tags[:n]

    def cache_refresh_apply(self, now: int, keys, kinds, acts, silos, tags, exts=None) -> np.ndarray:
        """ProcessCacheRefreshResponse in batch order; returns the per-item GD_CR_* status."""
        k = keys_array(keys)
        n = len(k)
        kind = np.ascontiguousarray(np.asarray(kinds, dtype=np.uint8))
        vals = np.zeros((max(n, 1), 2), dtype=np.uint32)
        vals[:n, 0] = acts
        vals[:n, 1] = silos
        t = np.ascontiguousarray(np.asarray(tags, dtype=np.int32))
        st = np.zeros(max(n, 1), dtype=np.uint8)
        x = None if exts is None else self._ext(exts, n)
        self._c(lib.gd_cache_refresh_apply(self.h, now, _ptr(k), None if x is None else C.byref(x.struct), _ptr(kind),
                                           _ptr(vals), _ptr(t), n, _ptr(st)))
        return st[:n]

    # -- follower fan-out ----------------------------------------------
    def fanout_route_bucket(self, row_off, dst, frontier, type_code: int, n_act: Optional[int]):
        """One publish hop (gd_fanout_route_bucket): returns dict of target, sender, status,
        silo, act (+ perm, offsets when n_act is not None)."""
        ro = np.ascontiguousarray(np.asarray(row_off, dtype=np.uint32))
        d = np.ascontiguousarray(np.asarray(dst, dtype=np.uint32))
        if d.size == 0:
            d = np.zeros(1, dtype=np.uint32)
        fr = np.ascontiguousarray(np.asarray(frontier, dtype=np.uint32))
        n_nodes = len(ro) - 1
        n = C.c_uint64(0)
        na = 0 if n_act is None else n_act
        # size query through the fused call with capacity 0 would do the work twice: count on the host
        valid = fr[fr < n_nodes]
        m = int((ro[valid.astype(np.int64) + 1].astype(np.int64) - ro[valid].astype(np.int64)).sum())
        out = {k: np.zeros(m, dtype=np.uint32) for k in ("target", "sender", "silo", "act")}
        out["status"] = np.zeros(m, dtype=np.uint8)
        perm = off = None
        if n_act is not None:
            perm = np.zeros(m, dtype=np.uint32)
            off = np.zeros(na + 2, dtype=np.uint32)
        P = lambda a: None if a is None else _ptr(a)  # noqa: E731
        self._c(lib.gd_fanout_route_bucket(self.h, _ptr(ro), _ptr(d), n_nodes, _ptr(fr) if len(fr) else None, len(fr),
                                           type_code, na, P(out["target"]), P(out["sender"]), P(out["silo"]),
                                           P(out["act"]), P(out["status"]), P(perm), P(off), m, C.byref(n)))
        assert n.value == m
        if n_act is not None:
            out["perm"], out["offsets"] = perm, off
        return out

    def fanout_expand_device(self, d_row_off: int, d_dst: int, n_nodes: int, d_frontier: int, n_frontier: int,
                             d_target: Optional[int], d_sender: Optional[int], capacity: int) -> int:
        n = C.c_uint64(0)
        self._c(lib.gd_fanout_expand_device(self.h, d_row_off, d_dst, n_nodes, d_frontier, n_frontier,
                                            d_target or None, d_sender or None, capacity, C.byref(n)))
        return n.value

    def fanout_route_bucket_device(self, d_row_off: int, d_dst: int, n_nodes: int, d_frontier: int, n_frontier: int,
                                   type_code: int, n_act: int, d_target: Optional[int], d_sender: int, d_silo: int,
                                   d_act: int, d_status: int, d_perm: Optional[int], d_offsets: Optional[int],
                                   capacity: int) -> int:
        n = C.c_uint64(0)
        self._c(lib.gd_fanout_route_bucket_device(self.h, d_row_off, d_dst, n_nodes, d_frontier, n_frontier, type_code,
                                                  n_act, d_target or None, d_sender, d_silo, d_act, d_status,
                                                  d_perm or None, d_offsets or None, capacity, C.byref(n)))
        return n.value

    def route_nodes_device(self, d_nodes: int, n: int, type_code: int, d_silo: int, d_act: int, d_status: int):
        self._c(lib.gd_route_nodes_device(self.h, d_nodes, n, type_code, d_silo, d_act, d_status))

    def pack_nodes_by_shard_device(self, d_nodes: int, d_payload: int, n: int, type_code: int, n_shards: int,
                                   d_send_nodes: int, d_send_payload: int, d_counts: int):
        self._c(lib.gd_pack_nodes_by_shard_device(self.h, d_nodes, d_payload, n, type_code, n_shards, d_send_nodes,
                                                  d_send_payload, d_counts))

    def frontier_next_device(self, d_offsets: int, n_act: int, d_visited: int, d_out: int) -> int:
        n = C.c_uint32(0)
        self._c(lib.gd_frontier_next_device(self.h, d_offsets, n_act, d_visited, d_out, C.byref(n)))
        return n.value

    # -- hot path (device pointers; enqueue only) -----------------------------------
    def route_device(self, d_keys: int, n: int, d_silo: int, d_act: int, d_status: int):
        self._c(lib.gd_route_device(self.h, C.c_void_p(d_keys), n, C.c_void_p(d_silo), C.c_void_p(d_act),
                                    C.c_void_p(d_status)))

    def route_bound_device(self, d_keys: int, n: int, d_silo: int, d_act: int, d_status: int):
        """gd_route_bound_device (diagnostic): the route kernel's memory bound over the 8-B index; the
        outputs are not route results."""
        self._c(lib.gd_route_bound_device(self.h, C.c_void_p(d_keys), n, C.c_void_p(d_silo), C.c_void_p(d_act),
                                          C.c_void_p(d_status)))

    def bucket_device(self, d_acts: int, n: int, n_act: int, d_perm: int, d_offsets: int):
        self._c(lib.gd_bucket_device(self.h, C.c_void_p(d_acts), n, n_act, C.c_void_p(d_perm), C.c_void_p(d_offsets)))

    def route_bucket_device(self, d_keys: int, n: int, n_act: int, d_silo: int, d_act: int, d_status: int,
                            d_perm: int, d_offsets: int):
        self._c(lib.gd_route_bucket_device(self.h, C.c_void_p(d_keys), n, n_act, C.c_void_p(d_silo),
                                           C.c_void_p(d_act), C.c_void_p(d_status), C.c_void_p(d_perm),
                                           C.c_void_p(d_offsets)))

    def ring_owner_device(self, d_keys: int, n: int, d_silo: int):
        self._c(lib.gd_ring_owner_device(self.h, C.c_void_p(d_keys), n, C.c_void_p(d_silo)))

    def pack_by_shard_device(self, d_keys: int, n: int, n_shards: int, d_send_keys: int, d_send_idx: int,
                             d_counts: int):
        self._c(lib.gd_pack_by_shard_device(self.h, C.c_void_p(d_keys), n, n_shards, C.c_void_p(d_send_keys),
                                            C.c_void_p(d_send_idx), C.c_void_p(d_counts)))

    def pack_routes_by_rank_device(self, d_keys: int, d_status: int, d_silo: int, n: int, n_shards: int, my_rank: int,
                                   d_send_keys: int, d_send_pos: int, d_counts: int):
        self._c(lib.gd_pack_routes_by_rank_device(self.h, C.c_void_p(d_keys), C.c_void_p(d_status), C.c_void_p(d_silo),
                                                  n, n_shards, my_rank, C.c_void_p(d_send_keys),
                                                  C.c_void_p(d_send_pos), C.c_void_p(d_counts)))

    # -- in-library exchange over RCCL (SURVEY 8 b gd_route_multi, 8 e) ----------------
    @staticmethod
    def comm_unique_id() -> bytes:
        buf = (C.c_uint8 * GD_COMM_ID_BYTES)()
        _check(None, lib.gd_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, unique_id: bytes, n_ranks: int, rank: int):
        assert len(unique_id) == GD_COMM_ID_BYTES
        buf = (C.c_uint8 * GD_COMM_ID_BYTES).from_buffer_copy(unique_id)
        self._c(lib.gd_comm_init(self.h, buf, n_ranks, rank))

    @staticmethod
    def comm_init_local(engines: Sequence["GrainDispatch"]):
        """gd_comm_init_local: the engines become ranks 0..W-1 of an in-process communicator (the
        W > 1 exchange rehearsed on one GPU; drive each engine from its own thread)."""
        arr = (C.c_void_p * len(engines))(*[e.h.value for e in engines])
        _check(None, lib.gd_comm_init_local(arr, len(engines)))

    def comm_destroy(self):
        self._c(lib.gd_comm_destroy(self.h))

    def route_multi_device(self, d_keys: int, n: int, n_act: int, return_routes: bool = False,
                           keys_ready: bool = False, forward: bool = False,
                           no_keys: bool = False) -> gd_multi_result:
        """Returns after the counts round; the rest is enqueued.  The result holds device pointers
        into library-owned buffers, valid through the next call (two batches in flight)."""
        r = gd_multi_result()
        flags = ((GD_MULTI_RETURN_ROUTES if return_routes else 0) | (GD_MULTI_KEYS_READY if keys_ready else 0)
                 | (GD_MULTI_FORWARD if forward else 0) | (GD_MULTI_NO_KEYS if no_keys else 0))
        self._c(lib.gd_route_multi_device(self.h, C.c_void_p(d_keys), n, n_act, flags, C.byref(r)))
        return r

    def route_multi(self, keys, n_act: int, return_routes: bool = False, forward: bool = False,
                    no_keys: bool = False) -> dict:
        """Host batch in, host results out (gd_route_multi + gd_multi_fetch)."""
        k = keys_array(keys)
        n = k.shape[0]
        r = gd_multi_result()
        flags = ((GD_MULTI_RETURN_ROUTES if return_routes else 0) | (GD_MULTI_FORWARD if forward else 0)
                 | (GD_MULTI_NO_KEYS if no_keys else 0))
        self._c(lib.gd_route_multi(self.h, _ptr(k), n, n_act, flags, C.byref(r)))
        return self.multi_fetch(r, n)

    # -- sharded fan-out cascade (gd_fanout_multi*) ------------------------------------
    def fanout_multi_device(self, d_row_off: int, d_dst: int, n_nodes: int, d_seeds: int, n_seeds: int,
                            type_code: int, n_act: int, hops: int):
        """gd_fanout_multi_device (collective over the communicator): a list of gd_fanout_hop with
        device pointers into library-owned buffers, valid until the next call."""
        out = (gd_fanout_hop * hops)()
        self._c(lib.gd_fanout_multi_device(self.h, C.c_void_p(d_row_off), C.c_void_p(d_dst), n_nodes,
                                           C.c_void_p(d_seeds or 0), n_seeds, type_code, n_act, hops, out))
        return list(out)

    def fanout_multi_part_device(self, d_row_off: int, d_dst: int, n_rows: int, d_node_of: int, d_seeds: int,
                                 n_seeds: int, type_code: int, hops: int):
        """gd_fanout_multi_part_device (collective): the cascade over this rank's partition of the
        follower graph (row i = local activation i, node d_node_of[i]); gd_fanout_hop list as
        fanout_multi_device (offsets over the n_rows local activations)."""
        out = (gd_fanout_hop * hops)()
        self._c(lib.gd_fanout_multi_part_device(self.h, C.c_void_p(d_row_off), C.c_void_p(d_dst or 0), n_rows,
                                                C.c_void_p(d_node_of or 0), C.c_void_p(d_seeds or 0), n_seeds,
                                                type_code, hops, out))
        return list(out)

    def fanout_cascade_device(self, d_row_off: int, d_dst: int, n_nodes: int, d_seeds: int, n_seeds: int,
                              type_code: int, n_act: int, hops: int):
        """gd_fanout_cascade_device: the one-GPU cascade inside the library; gd_fanout_hop list (device
        pointers into library buffers, src NULL), hops copied out with fanout_multi_fetch."""
        out = (gd_fanout_hop * hops)()
        self._c(lib.gd_fanout_cascade_device(self.h, C.c_void_p(d_row_off), C.c_void_p(d_dst or 0), n_nodes,
                                             C.c_void_p(d_seeds or 0), n_seeds, type_code, n_act, hops, out))
        return list(out)

    def fanout_multi(self, row_off, dst, seeds, type_code: int, n_act: int, hops: int) -> List[dict]:
        """gd_fanout_multi (host graph and seeds) + gd_fanout_multi_fetch of every hop."""
        ro = np.ascontiguousarray(row_off, dtype=np.uint32)
        d = np.ascontiguousarray(dst, dtype=np.uint32)
        sd = np.ascontiguousarray(seeds, dtype=np.uint32)
        out = (gd_fanout_hop * hops)()
        self._c(lib.gd_fanout_multi(self.h, _ptr(ro), _ptr(d) if d.size else None, len(ro) - 1,
                                    _ptr(sd) if sd.size else None, sd.size, type_code, n_act, hops, out))
        return [self.fanout_multi_fetch(i, out[i], n_act) for i in range(hops)]

    def fanout_multi_fetch(self, hop: int, r: gd_fanout_hop, n_act: int) -> dict:
        m = r.n_recv
        res = {"frontier": np.empty(r.n_frontier, np.uint32), "target": np.empty(m, np.uint32),
               "sender": np.empty(m, np.uint32), "src": np.empty(m, np.uint32), "silo": np.empty(m, np.uint32),
               "act": np.empty(m, np.uint32), "status": np.empty(m, np.uint8), "perm": np.empty(m, np.uint32),
               "offsets": np.empty(n_act + 2, np.uint32)}
        names = ("frontier", "target", "sender", "src", "silo", "act", "status", "perm", "offsets")
        self._c(lib.gd_fanout_multi_fetch(self.h, hop, *[C.c_void_p(_ptr(res[f])) if res[f].size else None
                                                         for f in names]))
        res["n_sent"] = int(r.n_sent)
        return res

    # -- multi-rank directory handoff (gd_dir_handoff_multi) ----------------------------
    def handoff_multi(self, keep_silos, n_silos: int, event: int, act_base: int) -> dict:
        """gd_dir_handoff_multi (collective) + gd_dir_handoff_fetch: the entries this rank received,
        in arrival order, with their activation index here, status and dropped address."""
        keep = self.keep_mask(keep_silos, n_silos)
        r = gd_handoff_result()
        self._c(lib.gd_dir_handoff_multi(self.h, _ptr(keep), len(keep), event, act_base, C.byref(r)))
        m = r.n_recv
        out = {"keys": np.empty((m, 3), np.uint64), "ids": np.empty((m, 3), np.uint64), "act": np.empty(m, np.uint32),
               "silo": np.empty(m, np.uint32), "src": np.empty(m, np.uint32), "status": np.empty(m, np.uint8),
               "dropped": np.empty((m, 2), np.uint32)}
        names = ("keys", "ids", "act", "silo", "src", "status", "dropped")
        self._c(lib.gd_dir_handoff_fetch(self.h, *[C.c_void_p(_ptr(out[f])) if m else None for f in names]))
        out["n_sent"] = int(r.n_sent)
        return out

    def split_ext(self, keep_silos, n_silos: int, move: bool = True):
        """gd_dir_split_ext: (keys (m,3) u64, acts, silos, KeyExt list (bytes / None)) in slot order."""
        keep = self.keep_mask(keep_silos, n_silos)
        n, nb = C.c_uint64(), C.c_uint64()
        self._c(lib.gd_dir_split_ext(self.h, _ptr(keep), len(keep), int(move), None, None, None, None, None, 0, 0,
                                     C.byref(n), C.byref(nb)))
        m = n.value
        keys = np.zeros((m, 3), np.uint64)
        vals = np.zeros((m, 2), np.uint32)
        off = np.zeros(m, np.uint64)
        ln = np.zeros(m, np.int32)
        blob = np.zeros(max(1, nb.value), np.uint8)
        if m:
            self._c(lib.gd_dir_split_ext(self.h, _ptr(keep), len(keep), int(move), _ptr(keys), _ptr(vals), _ptr(off),
                                         _ptr(ln), _ptr(blob), m, nb.value, C.byref(n), C.byref(nb)))
        exts = [None if ln[i] < 0 else bytes(blob[int(off[i]):int(off[i]) + int(ln[i])]) for i in range(m)]
        return keys, vals[:, 0].copy(), vals[:, 1].copy(), exts

    def ring_owner_ext(self, keys, exts) -> np.ndarray:
        k = keys_array(keys)
        n = len(k)
        x = self._ext(exts, n)
        out = np.zeros(n, dtype=np.uint32)
        self._c(lib.gd_ring_owner_ext(self.h, _ptr(k), C.byref(x.struct), n, _ptr(out)))
        return out

    def route_multi_ext(self, keys, exts, n_act: int, return_routes: bool = False, forward: bool = False) -> dict:
        """route_multi with KeyExt grains routed on their owner (strings travel with the batch)."""
        k = keys_array(keys)
        n = k.shape[0]
        x = self._ext(exts, n)
        r = gd_multi_result()
        flags = (GD_MULTI_RETURN_ROUTES if return_routes else 0) | (GD_MULTI_FORWARD if forward else 0)
        self._c(lib.gd_route_multi_ext(self.h, _ptr(k), C.byref(x.struct), n, n_act, flags, C.byref(r)))
        return self.multi_fetch(r, n)

    def multi_fetch(self, r: gd_multi_result, n: int) -> dict:
        """Host copies of the last gd_route_multi* result (n = this rank's batch size)."""
        m = r.n_recv
        out = {"recv_keys": np.empty((m, 3), np.uint64) if r.recv_keys else None, "recv_idx": np.empty(m, np.uint32),
               "recv_src": np.empty(m, np.uint32), "silo": np.empty(m, np.uint32), "act": np.empty(m, np.uint32),
               "status": np.empty(m, np.uint8), "perm": np.empty(m, np.uint32),
               "offsets": np.empty(r.n_act + 2, np.uint32)}
        if r.ret_silo:
            out.update(ret_silo=np.empty(n, np.uint32), ret_act=np.empty(n, np.uint32), ret_status=np.empty(n, np.uint8))
        names = ("recv_keys", "recv_idx", "recv_src", "silo", "act", "status", "perm", "offsets", "ret_silo",
                 "ret_act", "ret_status")
        self._c(lib.gd_multi_fetch(self.h, *[C.c_void_p(_ptr(out[f])) if out.get(f) is not None else None
                                             for f in names]))
        return out

    # -- header decode -------------------------------------------------
    @staticmethod
    def _frame_host(n: int, fields) -> Tuple[dict, gd_frame_fields]:
        want = set(FRAME_FIELDS) if fields is None else {"flags", "target_grain", *fields}
        arrs = {k: np.zeros((n,) + FRAME_FIELDS[k][1], dtype=FRAME_FIELDS[k][0]) for k in want}
        ff = gd_frame_fields(**{k: (_ptr(a) if n else None) for k, a in arrs.items()})
        return arrs, ff

    def decode_frames(self, buf: bytes, offsets, fields: Optional[Iterable[str]] = None) -> dict:
        """Decode the frames starting at `offsets` in `buf` (host bytes).  Returns a dict of
        numpy arrays named like gd_frame_fields (all fields unless `fields` narrows it)."""
        b = np.frombuffer(buf, dtype=np.uint8) if len(buf) else np.zeros(1, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        n = len(off)
        arrs, ff = self._frame_host(n, fields)
        self._c(lib.gd_decode_frames(self.h, _ptr(b), len(buf), _ptr(off), n, C.byref(ff)))
        return arrs

    def route_frames(self, buf: bytes, offsets, n_act: Optional[int] = None, fields: Optional[Iterable[str]] = (),
                     keyext: bool = False):
        """Decode -> route (-> bucket when n_act is given).  Returns (decoded fields, status,
        silo, act[, perm, offsets]).  keyext: gd_route_frames_ext (KeyExt targets routed too)."""
        b = np.frombuffer(buf, dtype=np.uint8) if len(buf) else np.zeros(1, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        n = len(off)
        arrs, ff = self._frame_host(n, fields)
        silo = np.zeros(n, dtype=np.uint32)
        act = np.zeros(n, dtype=np.uint32)
        st = np.zeros(n, dtype=np.uint8)
        perm = np.zeros(n, dtype=np.uint32) if n_act is not None else None
        offs = np.zeros(n_act + 2, dtype=np.uint32) if n_act is not None else None
        fn = lib.gd_route_frames_ext if keyext else lib.gd_route_frames
        self._c(fn(self.h, _ptr(b), len(buf), _ptr(off), n, n_act or 0, C.byref(ff), _ptr(silo),
                   _ptr(act), _ptr(st), None if perm is None else _ptr(perm), None if offs is None else _ptr(offs)))
        return (arrs, st, silo, act) if n_act is None else (arrs, st, silo, act, perm, offs)

    def decode_frames_device(self, d_buf: int, buf_len: int, d_offsets: int, n: int, d_fields: dict):
        ff = gd_frame_fields(**{k: C.c_void_p(v) for k, v in d_fields.items()})
        self._c(lib.gd_decode_frames_device(self.h, C.c_void_p(d_buf), buf_len, C.c_void_p(d_offsets), n,
                                            C.byref(ff)))

    def route_frames_device(self, d_buf: int, buf_len: int, d_offsets: int, n: int, n_act: int, d_fields: dict,
                            d_silo: int, d_act: int, d_status: int, d_perm: Optional[int], d_offs: Optional[int]):
        ff = gd_frame_fields(**{k: C.c_void_p(v) for k, v in d_fields.items()})
        self._c(lib.gd_route_frames_device(self.h, C.c_void_p(d_buf), buf_len, C.c_void_p(d_offsets), n, n_act,
                                           C.byref(ff), C.c_void_p(d_silo), C.c_void_p(d_act), C.c_void_p(d_status),
                                           C.c_void_p(d_perm or 0), C.c_void_p(d_offs or 0)))

    # -- frame encoder (Message.SetTargetPlacement + Message.Serialize) -----------------
    def encode_configure(self, silos: Sequence[Tuple[str, int, int]], type_names: Sequence[str] = ()):
        """gd_encode_configure: silos[s] = (ip, port, generation) of silo index s; type_names[t] = the
        grain-class name new_type index t stands for."""
        arr = (gd_silo_addr * len(silos))(*[silo_addr(*s) for s in silos])
        blobs = [t.encode("utf-8") for t in type_names]
        off = np.zeros(len(blobs) + 1, np.uint32)
        off[1:] = np.cumsum([len(b) for b in blobs], dtype=np.uint64)
        utf8 = np.frombuffer(b"".join(blobs) or b"\0", dtype=np.uint8)
        self._c(lib.gd_encode_configure(self.h, arr, len(silos), _ptr(utf8), _ptr(off), len(blobs)))

    def encode_frames(self, buf: bytes, offsets, silo, act, status, placed=None, new_type=None, order=None,
                      out_cap: Optional[int] = None, out: Optional[np.ndarray] = None):
        """gd_encode_frames: (out bytes u8[out_cap], out_off u64[n + 1], enc_status u8[n], total).  `out`: a
        caller's u8 array to write into (its length is out_cap)."""
        b = np.frombuffer(buf, dtype=np.uint8) if len(buf) else np.zeros(1, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        n = len(off)
        s = np.ascontiguousarray(np.asarray(silo, dtype=np.uint32))
        a = np.ascontiguousarray(np.asarray(act, dtype=np.uint32))
        st = np.ascontiguousarray(np.asarray(status, dtype=np.uint8))
        pl, nt, od = self._opt(placed, np.uint8), self._opt(new_type, np.uint32), self._opt(order, np.uint32)
        if out is None:
            out = np.zeros(len(buf) + n * 128 if out_cap is None else out_cap, np.uint8)
        out_off = np.zeros(n + 1, np.uint64)
        est = np.zeros(n, np.uint8)
        total = C.c_uint64(0)
        self._c(lib.gd_encode_frames(self.h, _ptr(b), len(buf), _ptr(off), n, _ptr(s), _ptr(a), _ptr(st),
                                     None if pl is None else _ptr(pl), None if nt is None else _ptr(nt),
                                     None if od is None else _ptr(od), _ptr(out) if len(out) else None, len(out),
                                     _ptr(out_off), _ptr(est), C.byref(total)))
        return out, out_off, est, int(total.value)

    def encode_frames_device(self, d_buf: int, buf_len: int, d_offsets: int, n: int, d_silo: int, d_act: int,
                             d_status: int, d_placed: Optional[int], d_new_type: Optional[int],
                             d_order: Optional[int], d_out: int, out_cap: int, d_out_off: int, d_enc_status: int):
        self._c(lib.gd_encode_frames_device(self.h, C.c_void_p(d_buf), buf_len, C.c_void_p(d_offsets), n,
                                            C.c_void_p(d_silo), C.c_void_p(d_act), C.c_void_p(d_status),
                                            C.c_void_p(d_placed or 0), C.c_void_p(d_new_type or 0),
                                            C.c_void_p(d_order or 0), C.c_void_p(d_out), out_cap,
                                            C.c_void_p(d_out_off), C.c_void_p(d_enc_status)))

    # -- response writer (CreateResponseMessage / CreateRejectionResponse + Message.Serialize) ------
    def respond_configure(self, infos: Sequence[str] = ()):
        """gd_respond_configure: infos[k] = the RejectionInfo string info index k stands for."""
        blobs = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in infos]
        off = np.zeros(len(blobs) + 1, np.uint32)
        off[1:] = np.cumsum([len(b) for b in blobs], dtype=np.uint64)
        utf8 = np.frombuffer(b"".join(blobs) or b"\0", dtype=np.uint8)
        self._c(lib.gd_respond_configure(self.h, _ptr(utf8), _ptr(off), len(blobs)))

    def respond_kinds(self, turn, recv_status=None):
        """gd_respond_kinds: (kind u8[n], rejection_type u8[n])."""
        t = np.ascontiguousarray(np.asarray(turn, dtype=np.uint8))
        r = self._opt(recv_status, np.uint8)
        n = len(t)
        kind, rej = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        self._c(lib.gd_respond_kinds(self.h, _ptr(t), None if r is None else _ptr(r), n, _ptr(kind), _ptr(rej)))
        return kind, rej

    def respond_kinds_device(self, d_turn: int, d_recv_status: Optional[int], n: int, d_kind: int,
                             d_rejection_type: int):
        self._c(lib.gd_respond_kinds_device(self.h, C.c_void_p(d_turn), C.c_void_p(d_recv_status or 0), n,
                                            C.c_void_p(d_kind), C.c_void_p(d_rejection_type)))

    def silo_index(self, wire24):
        """gd_silo_index: wire24 = (n, 24) u8 wire SiloAddresses -> silo index u32[n] (NO_SILO: not in the table)."""
        w = np.ascontiguousarray(np.asarray(wire24, dtype=np.uint8).reshape(-1, 24))
        n = len(w)
        silo = np.zeros(n, np.uint32)
        self._c(lib.gd_silo_index(self.h, _ptr(w) if n else None, n, _ptr(silo) if n else None))
        return silo

    def silo_index_device(self, d_wire24: int, n: int, d_silo: int):
        self._c(lib.gd_silo_index_device(self.h, C.c_void_p(d_wire24), n, C.c_void_p(d_silo)))

    def respond_frames(self, buf: bytes, offsets, kind, result=None, rejection_type=None, info=None, body=None,
                       body_off=None, order=None, out_cap: Optional[int] = None, out: Optional[np.ndarray] = None):
        """gd_respond_frames: (out bytes u8[out_cap], out_off u64[n + 1], rsp_status u8[n], total).  `out`: a
        caller's u8 array to write into (its length is out_cap)."""
        b = np.frombuffer(buf, dtype=np.uint8) if len(buf) else np.zeros(1, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        n = len(off)
        k = np.ascontiguousarray(np.asarray(kind, dtype=np.uint8))
        rs, rt, inf = self._opt(result, np.uint8), self._opt(rejection_type, np.uint8), self._opt(info, np.uint32)
        bo, od = self._opt(body_off, np.uint64), self._opt(order, np.uint32)
        bd = None
        if body is not None and bo is not None:
            bd = np.frombuffer(bytes(body), dtype=np.uint8) if len(body) else np.zeros(1, dtype=np.uint8)
        nbody = int(bo[-1]) if bd is not None and len(bo) else 0
        if out is None:
            out = np.zeros(len(buf) + nbody + n * (16 + 256) if out_cap is None else out_cap, np.uint8)
        out_off = np.zeros(n + 1, np.uint64)
        st = np.zeros(n, np.uint8)
        total = C.c_uint64(0)
        p = lambda a: None if a is None else _ptr(a)
        self._c(lib.gd_respond_frames(self.h, _ptr(b), len(buf), _ptr(off), n, _ptr(k), p(rs), p(rt), p(inf), p(bd),
                                      p(bo) if bd is not None else None, p(od), _ptr(out) if len(out) else None,
                                      len(out), _ptr(out_off), _ptr(st), C.byref(total)))
        return out, out_off, st, int(total.value)

    def respond_frames_device(self, d_buf: int, buf_len: int, d_offsets: int, n: int, d_kind: int,
                              d_result: Optional[int], d_rejection_type: Optional[int], d_info: Optional[int],
                              d_body: Optional[int], d_body_off: Optional[int], d_order: Optional[int], d_out: int,
                              out_cap: int, d_out_off: int, d_rsp_status: int):
        v = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_respond_frames_device(self.h, v(d_buf), buf_len, v(d_offsets), n, v(d_kind), v(d_result),
                                             v(d_rejection_type), v(d_info), v(d_body), v(d_body_off), v(d_order),
                                             v(d_out), out_cap, v(d_out_off), v(d_rsp_status)))

    # -- request writer (CreateMessage + SendRequest + SetTargetPlacement + Message.Serialize) -------
    def request_configure(self, strings: Sequence[str] = ()):
        """gd_request_configure: strings[k] = the DebugContext / GenericGrainType string index k stands for."""
        blobs = [t.encode("utf-8") if isinstance(t, str) else bytes(t) for t in strings]
        off = np.zeros(len(blobs) + 1, np.uint32)
        off[1:] = np.cumsum([len(b) for b in blobs], dtype=np.uint64)
        utf8 = np.frombuffer(b"".join(blobs) or b"\0", dtype=np.uint8)
        self._c(lib.gd_request_configure(self.h, _ptr(utf8), _ptr(off), len(blobs)))

    def _request_batch(self, target, sender_grain, sender_act, target_ext=None, sender_ext=None, options=None,
                       generic=None, debug=None, id_base: int = 0, ttl_ticks: int = TTL_NONE, body=None,
                       body_off=None):
        """(gd_request_batch with host pointers, n, body bytes, the arrays it points at).  target_ext / sender_ext:
        a KeyExtBatch or a list of its items."""
        tg, sg = keys_array(target), keys_array(sender_grain)
        n = len(tg)
        sa = np.ascontiguousarray(np.asarray(sender_act, dtype=np.uint32))
        tx = target_ext if target_ext is None or isinstance(target_ext, KeyExtBatch) else KeyExtBatch(target_ext)
        sx = sender_ext if sender_ext is None or isinstance(sender_ext, KeyExtBatch) else KeyExtBatch(sender_ext)
        op, ge, db = self._opt(options, np.uint8), self._opt(generic, np.uint32), self._opt(debug, np.uint32)
        bo = self._opt(body_off, np.uint64)
        bd = None
        if body is not None and bo is not None:
            bd = np.frombuffer(bytes(body), dtype=np.uint8) if len(body) else np.zeros(1, dtype=np.uint8)
        p = lambda a: None if a is None else _ptr(a)
        b = gd_request_batch(_ptr(tg), None if tx is None else C.pointer(tx.struct), _ptr(sg),
                             None if sx is None else C.pointer(sx.struct), _ptr(sa), p(op), p(ge), p(db), id_base,
                             ttl_ticks, p(bd), p(bo) if bd is not None else None)
        nbody = int(bo[-1]) if bd is not None and len(bo) else 0
        return b, n, nbody + sum(int(x.blob.size) for x in (tx, sx) if x is not None), (tg, sg, sa, tx, sx, op, ge, db, bd, bo)

    def request_frames(self, batch: dict, silo=None, act=None, status=None, placed=None, new_type=None, order=None,
                       out_cap: Optional[int] = None, out: Optional[np.ndarray] = None):
        """gd_request_frames: (out bytes u8[out_cap], out_off u64[n + 1], req_status u8[n], total).  batch: the
        keyword arguments of _request_batch."""
        b, n, extra, keep = self._request_batch(**batch)
        sl, ac, st = self._opt(silo, np.uint32), self._opt(act, np.uint32), self._opt(status, np.uint8)
        pl, nt, od = self._opt(placed, np.uint8), self._opt(new_type, np.uint32), self._opt(order, np.uint32)
        if out is None:
            out = np.zeros(extra + n * 512 if out_cap is None else out_cap, np.uint8)
        out_off = np.zeros(n + 1, np.uint64)
        rst = np.zeros(n, np.uint8)
        total = C.c_uint64(0)
        p = lambda a: None if a is None else _ptr(a)
        self._c(lib.gd_request_frames(self.h, C.byref(b), n, p(sl), p(ac), p(st), p(pl), p(nt), p(od),
                                      _ptr(out) if len(out) else None, len(out), _ptr(out_off), _ptr(rst),
                                      C.byref(total)))
        return out, out_off, rst, int(total.value)

    @staticmethod
    def _request_batch_device(d: dict):
        """gd_request_batch from device addresses; target_ext / sender_ext: (d_bytes, d_offset, d_length, bytes_len)."""
        v = lambda k: d.get(k) or None
        exts = [None if d.get(k) is None else gd_key_ext(*d[k]) for k in ("target_ext", "sender_ext")]
        b = gd_request_batch(v("target"), None if exts[0] is None else C.pointer(exts[0]), v("sender_grain"),
                             None if exts[1] is None else C.pointer(exts[1]), v("sender_act"), v("options"),
                             v("generic"), v("debug"), d.get("id_base", 0), d.get("ttl_ticks", TTL_NONE), v("body"),
                             v("body_off"))
        return b, exts

    def request_frames_device(self, d_batch: dict, n: int, d_silo: Optional[int], d_act: Optional[int],
                              d_status: Optional[int], d_placed: Optional[int], d_new_type: Optional[int],
                              d_order: Optional[int], d_out: int, out_cap: int, d_out_off: int, d_req_status: int):
        b, keep = self._request_batch_device(d_batch)
        v = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_request_frames_device(self.h, C.byref(b), n, v(d_silo), v(d_act), v(d_status), v(d_placed),
                                             v(d_new_type), v(d_order), v(d_out), out_cap, v(d_out_off),
                                             v(d_req_status)))

    def request_send(self, batch: dict, out_cap: Optional[int] = None, out: Optional[np.ndarray] = None) -> dict:
        """gd_request_send: route + sender queues + writer; a dict of every stage's outputs."""
        b, n, extra, keep = self._request_batch(**batch)
        silo, act, perm = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        status, sst, rst = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        q = np.zeros(n, np.uint32)
        offsets = np.zeros(getattr(self, "send_n_queues", 0) + 5, np.uint32)   # GD_ESTATE before send_configure
        if out is None:
            out = np.zeros(extra + n * 512 if out_cap is None else out_cap, np.uint8)
        out_off = np.zeros(n + 1, np.uint64)
        total = C.c_uint64(0)
        self._c(lib.gd_request_send(self.h, C.byref(b), n, _ptr(silo), _ptr(act), _ptr(status), _ptr(sst), _ptr(q),
                                    _ptr(perm), _ptr(offsets), _ptr(out) if len(out) else None, len(out),
                                    _ptr(out_off), _ptr(rst), C.byref(total)))
        return {"silo": silo, "act": act, "status": status, "send_status": sst, "queue": q, "perm": perm,
                "offsets": offsets, "out": out, "out_off": out_off, "req_status": rst, "total": int(total.value)}

    def request_send_device(self, d_batch: dict, n: int, d_silo: int, d_act: int, d_status: int, d_send_status: int,
                            d_queue: Optional[int], d_perm: int, d_offsets: int, d_out: int, out_cap: int,
                            d_out_off: int, d_req_status: int):
        b, keep = self._request_batch_device(d_batch)
        v = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_request_send_device(self.h, C.byref(b), n, v(d_silo), v(d_act), v(d_status), v(d_send_status),
                                           v(d_queue), v(d_perm), v(d_offsets), v(d_out), out_cap, v(d_out_off),
                                           v(d_req_status)))

    # -- forward writer (TryForwardRequest + AddressMessage + Message.Serialize) -------------------
    def forward_kinds(self, turn):
        """gd_forward_kinds: kind u8[n]."""
        t = np.ascontiguousarray(np.asarray(turn, dtype=np.uint8))
        kind = np.zeros(len(t), np.uint8)
        self._c(lib.gd_forward_kinds(self.h, _ptr(t), len(t), _ptr(kind)))
        return kind

    def forward_kinds_device(self, d_turn: int, n: int, d_kind: int):
        self._c(lib.gd_forward_kinds_device(self.h, C.c_void_p(d_turn), n, C.c_void_p(d_kind)))

    def _forward_batch(self, buf: bytes, offsets, kind, old_act=None, fwd_silo=None, fwd_act=None,
                       max_forward_count: int = 2, local_silo: int = 0):
        """(gd_forward_batch with host pointers, n, the arrays it points at)."""
        b = np.frombuffer(buf, dtype=np.uint8) if len(buf) else np.zeros(1, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        k = np.ascontiguousarray(np.asarray(kind, dtype=np.uint8))
        oa, fs, fa = self._opt(old_act, np.uint32), self._opt(fwd_silo, np.uint32), self._opt(fwd_act, np.uint32)
        p = lambda a: None if a is None else _ptr(a)
        fb = gd_forward_batch(_ptr(b), len(buf), _ptr(off), _ptr(k), p(oa), p(fs), p(fa), max_forward_count,
                              local_silo)
        return fb, len(off), (b, off, k, oa, fs, fa)

    def forward_frames(self, batch: dict, silo=None, act=None, status=None, placed=None, new_type=None, order=None,
                       out_cap: Optional[int] = None, out: Optional[np.ndarray] = None):
        """gd_forward_frames: (out bytes u8[out_cap], out_off u64[n + 1], fwd_status u8[n], target u64[n, 3], total).
        batch: the keyword arguments of _forward_batch."""
        fb, n, keep = self._forward_batch(**batch)
        sl, ac, st = self._opt(silo, np.uint32), self._opt(act, np.uint32), self._opt(status, np.uint8)
        pl, nt, od = self._opt(placed, np.uint8), self._opt(new_type, np.uint32), self._opt(order, np.uint32)
        if out is None:
            out = np.zeros(2 * len(batch["buf"]) + n * 256 if out_cap is None else out_cap, np.uint8)
        out_off = np.zeros(n + 1, np.uint64)
        fst = np.zeros(n, np.uint8)
        target = np.zeros((n, 3), np.uint64)
        total = C.c_uint64(0)
        p = lambda a: None if a is None else _ptr(a)
        self._c(lib.gd_forward_frames(self.h, C.byref(fb), n, p(sl), p(ac), p(st), p(pl), p(nt), p(od),
                                      _ptr(out) if len(out) else None, len(out), _ptr(out_off), _ptr(fst),
                                      _ptr(target) if n else None, C.byref(total)))
        return out, out_off, fst, target, int(total.value)

    @staticmethod
    def _forward_batch_device(d: dict):
        v = lambda k: d.get(k) or None
        return gd_forward_batch(v("buf"), d.get("buf_len", 0), v("frame_off"), v("kind"), v("old_act"), v("fwd_silo"),
                                v("fwd_act"), d.get("max_forward_count", 2), d.get("local_silo", 0))

    def forward_frames_device(self, d_batch: dict, n: int, d_silo: Optional[int], d_act: Optional[int],
                              d_status: Optional[int], d_placed: Optional[int], d_new_type: Optional[int],
                              d_order: Optional[int], d_out: int, out_cap: int, d_out_off: int, d_fwd_status: int,
                              d_target: Optional[int]):
        """d_batch: device addresses under _forward_batch's names, plus buf_len."""
        fb = self._forward_batch_device(d_batch)
        v = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_forward_frames_device(self.h, C.byref(fb), n, v(d_silo), v(d_act), v(d_status), v(d_placed),
                                             v(d_new_type), v(d_order), v(d_out), out_cap, v(d_out_off),
                                             v(d_fwd_status), v(d_target)))

    def forward_reject_frames(self, batch: dict, info=None, body=None, body_off=None, order=None,
                              out_cap: Optional[int] = None, out: Optional[np.ndarray] = None):
        """gd_forward_reject_frames: (out bytes u8[out_cap], out_off u64[n + 1], rej_status u8[n], total).  batch:
        the keyword arguments of _forward_batch (fwd_silo / fwd_act are ignored)."""
        fb, n, keep = self._forward_batch(**batch)
        inf, bo, od = self._opt(info, np.uint32), self._opt(body_off, np.uint64), self._opt(order, np.uint32)
        bd = None
        if body is not None and bo is not None:
            bd = np.frombuffer(bytes(body), dtype=np.uint8) if len(body) else np.zeros(1, dtype=np.uint8)
        nbody = int(bo[-1]) if bd is not None and len(bo) else 0
        if out is None:
            out = np.zeros(2 * len(batch["buf"]) + nbody + n * (90 + 256) if out_cap is None else out_cap, np.uint8)
        out_off = np.zeros(n + 1, np.uint64)
        st = np.zeros(n, np.uint8)
        total = C.c_uint64(0)
        p = lambda a: None if a is None else _ptr(a)
        self._c(lib.gd_forward_reject_frames(self.h, C.byref(fb), n, p(inf), p(bd), p(bo) if bd is not None else None,
                                             p(od), _ptr(out) if len(out) else None, len(out), _ptr(out_off),
                                             _ptr(st), C.byref(total)))
        return out, out_off, st, int(total.value)

    def forward_reject_frames_device(self, d_batch: dict, n: int, d_info: Optional[int], d_body: Optional[int],
                                     d_body_off: Optional[int], d_order: Optional[int], d_out: int, out_cap: int,
                                     d_out_off: int, d_rej_status: int):
        """d_batch: device addresses under _forward_batch's names, plus buf_len."""
        fb = self._forward_batch_device(d_batch)
        v = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_forward_reject_frames_device(self.h, C.byref(fb), n, v(d_info), v(d_body), v(d_body_off),
                                                    v(d_order), v(d_out), out_cap, v(d_out_off), v(d_rej_status)))

    def forward_send(self, batch: dict, out_cap: Optional[int] = None, out: Optional[np.ndarray] = None) -> dict:
        """gd_forward_send: plan + route + sender queues + writer; a dict of every stage's outputs."""
        fb, n, keep = self._forward_batch(**batch)
        silo, act, perm = np.zeros(n, np.uint32), np.zeros(n, np.uint32), np.zeros(n, np.uint32)
        status, sst, fst = np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        q = np.zeros(n, np.uint32)
        offsets = np.zeros(getattr(self, "send_n_queues", 0) + 5, np.uint32)   # GD_ESTATE before send_configure
        if out is None:
            out = np.zeros(2 * len(batch["buf"]) + n * 256 if out_cap is None else out_cap, np.uint8)
        out_off = np.zeros(n + 1, np.uint64)
        target = np.zeros((max(n, 1), 3), np.uint64)
        total = C.c_uint64(0)
        self._c(lib.gd_forward_send(self.h, C.byref(fb), n, _ptr(silo), _ptr(act), _ptr(status), _ptr(sst), _ptr(q),
                                    _ptr(perm), _ptr(offsets), _ptr(out) if len(out) else None, len(out),
                                    _ptr(out_off), _ptr(fst), _ptr(target), C.byref(total)))
        return {"silo": silo, "act": act, "status": status, "send_status": sst, "queue": q, "perm": perm,
                "offsets": offsets, "out": out, "out_off": out_off, "fwd_status": fst, "target": target[:n],
                "total": int(total.value)}

    def forward_send_device(self, d_batch: dict, n: int, d_silo: int, d_act: int, d_status: int, d_send_status: int,
                            d_queue: Optional[int], d_perm: int, d_offsets: int, d_out: int, out_cap: int,
                            d_out_off: int, d_fwd_status: int, d_target: int):
        fb = self._forward_batch_device(d_batch)
        v = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_forward_send_device(self.h, C.byref(fb), n, v(d_silo), v(d_act), v(d_status), v(d_send_status),
                                           v(d_queue), v(d_perm), v(d_offsets), v(d_out), out_cap, v(d_out_off),
                                           v(d_fwd_status), v(d_target)))

    # -- sniff stage (SniffIncomingMessage + InvalidateCacheEntry) -------------------------------
    @staticmethod
    def _sniff_host(n: int, ent_cap: int):
        """(gd_sniff_out with host pointers, the arrays it points at by field name)."""
        a = {"count": np.zeros(n, np.uint32), "ent_off": np.zeros(n + 1, np.uint32), "status": np.zeros(n, np.uint8),
             "flags": np.zeros(n, np.uint8), "ent_frame": np.zeros(ent_cap, np.uint32),
             "ent_silo": np.zeros((ent_cap, 6), np.uint32), "ent_grain": np.zeros((ent_cap, 3), np.uint64),
             "ent_ext_off": np.zeros(ent_cap, np.uint64), "ent_ext_len": np.zeros(ent_cap, np.int32),
             "ent_act_id": np.zeros((ent_cap, 3), np.uint64)}
        one = np.zeros(4, np.uint64)                           # what an empty array's pointer stands on
        return gd_sniff_out(*[_ptr(a[f]) if a[f].size else _ptr(one) for f in SNIFF_FIELDS]), dict(a, _one=one)

    @staticmethod
    def _sniff_result(a: dict, m: int) -> dict:
        out = {f: (v[:m] if f.startswith("ent_") and f != "ent_off" else v) for f, v in a.items() if f != "_one"}
        out["m"] = m
        return out

    def sniff_frames(self, buf: bytes, offsets, ent_cap: Optional[int] = None) -> dict:
        """gd_sniff_frames: the per-frame arrays, the first m entries of the per-entry arrays, and m.
        ent_cap None: len(buf) // 80, the most a buffer can hold."""
        b = np.frombuffer(buf, dtype=np.uint8) if len(buf) else np.zeros(1, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        n = len(off)
        cap = len(buf) // 80 if ent_cap is None else ent_cap
        so, a = self._sniff_host(n, cap)
        m = C.c_uint32(0)
        try:
            self._c(lib.gd_sniff_frames(self.h, _ptr(b), len(buf), _ptr(off) if n else None, n, C.byref(so), cap,
                                        C.byref(m)))
        except GrainDispatchError as ex:                       # GD_EFULL: ent_off is complete, the entry arrays untouched
            ex.arrays = a
            raise
        return self._sniff_result(a, int(m.value))

    def sniff_frames_device(self, d_buf: int, buf_len: int, d_offsets: int, n: int, d_out: dict, ent_cap: int):
        """d_out: device addresses under gd_sniff_out's field names (absent or None: not wanted)."""
        so = gd_sniff_out(*[d_out.get(f) or None for f in SNIFF_FIELDS])
        self._c(lib.gd_sniff_frames_device(self.h, C.c_void_p(d_buf or 0), buf_len, C.c_void_p(d_offsets or 0), n,
                                           C.byref(so), ent_cap))

    def cache_invalidate(self, keys, act_ids, exts=None) -> np.ndarray:
        """gd_cache_invalidate: InvalidateCacheEntry(keys[k], act_ids[k]) in order; out u8[m] of GD_INV_*."""
        k, ids = keys_array(keys), keys_array(act_ids)
        m = len(k)
        assert len(ids) == m, "one ActivationId per key"
        out = np.zeros(m, np.uint8)
        x = None if exts is None else self._ext(exts, m)
        self._c(lib.gd_cache_invalidate(self.h, _ptr(k), None if x is None else C.byref(x.struct), _ptr(ids), m,
                                        _ptr(out)))
        return out

    def cache_invalidate_device(self, d_keys: int, d_ext: Optional[dict], d_act_ids: int, m: int, d_m: Optional[int],
                                d_out: int):
        """d_ext: {"bytes", "offset", "length", "bytes_len"} of device addresses, or None."""
        dx = None if d_ext is None else gd_key_ext(d_ext.get("bytes") or None, d_ext["offset"], d_ext["length"],
                                                   d_ext.get("bytes_len", 0))
        v = lambda a: C.c_void_p(a or 0)
        self._c(lib.gd_cache_invalidate_device(self.h, v(d_keys), None if dx is None else C.byref(dx), v(d_act_ids), m,
                                               v(d_m), v(d_out)))

    def sniff_invalidate(self, buf: bytes, offsets, ent_cap: Optional[int] = None) -> dict:
        """gd_sniff_invalidate: sniff_frames' dict plus "inv" u8[m] of GD_INV_*."""
        b = np.frombuffer(buf, dtype=np.uint8) if len(buf) else np.zeros(1, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        n = len(off)
        cap = len(buf) // 80 if ent_cap is None else ent_cap
        so, a = self._sniff_host(n, cap)
        inv = np.zeros(cap, np.uint8)
        m = C.c_uint32(0)
        try:
            self._c(lib.gd_sniff_invalidate(self.h, _ptr(b), len(buf), _ptr(off) if n else None, n, C.byref(so), cap,
                                            _ptr(inv) if cap else None, C.byref(m)))
        except GrainDispatchError as ex:
            ex.arrays = dict(a, inv=inv)
            raise
        out = self._sniff_result(a, int(m.value))
        out["inv"] = inv[:out["m"]]
        return out

    def sniff_invalidate_device(self, d_buf: int, buf_len: int, d_offsets: int, n: int, d_out: dict, ent_cap: int,
                                d_inv: int):
        so = gd_sniff_out(*[d_out.get(f) or None for f in SNIFF_FIELDS])
        self._c(lib.gd_sniff_invalidate_device(self.h, C.c_void_p(d_buf or 0), buf_len, C.c_void_p(d_offsets or 0), n,
                                               C.byref(so), ent_cap, C.c_void_p(d_inv or 0)))

    # -- batched Catalog.GetOrCreateActivation -----------------------------------------
    def activate(self, ctx, recv_status, target_activation, n_ctx: int, cap_new: int, ctx_base: int = 0, new_ctx=None,
                 direction=None, ttl=None, new_placement=None, terminating: bool = False, target_grain=None,
                 lists: bool = True) -> dict:
        """gd_activate: kind u8, ctx u32, status u8, n_proposed[, new_idx u32[n_new], gone_idx u32[n_gone]].  A
        refused batch raises GD_EINVAL with the outputs in the error's `arrays`."""
        c = np.ascontiguousarray(np.asarray(ctx, dtype=np.uint32))
        n = len(c)
        rs = np.ascontiguousarray(np.asarray(recv_status, dtype=np.uint8))
        ta = keys_array(target_activation)
        tg = None if target_grain is None else keys_array(target_grain)
        dr, tl = self._opt(direction, np.uint8), self._opt(ttl, np.int64)
        npl, nc = self._opt(new_placement, np.uint8), self._opt(new_ctx, np.uint32)
        kind, co, so = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        new_idx = np.zeros(max(n, 1), np.uint32) if lists else None
        gone_idx = np.zeros(max(n, 1), np.uint32) if lists else None
        words = np.zeros(3, np.uint32)                       # n_new, n_gone, n_proposed
        p = lambda a: None if a is None else _ptr(a)
        w = lambda k: words.ctypes.data + 4 * k

        def result():
            out = dict(kind=kind, ctx=co, status=so, n_proposed=int(words[2]))
            if lists:
                out.update(new_idx=new_idx[:int(words[0])].copy(), gone_idx=gone_idx[:int(words[1])].copy())
            return out
        try:
            self._c(lib.gd_activate(self.h, _ptr(c), _ptr(rs), p(tg), _ptr(ta), p(dr), p(tl), p(npl), n, n_ctx,
                                    int(terminating), ctx_base, p(nc), cap_new, _ptr(kind), _ptr(co), _ptr(so),
                                    p(new_idx), w(0) if lists else None, p(gone_idx), w(1) if lists else None, w(2)))
        except GrainDispatchError as ex:
            ex.arrays = result()
            raise
        return result()

    def activate_device(self, d_ctx: int, d_recv_status: int, d_target_activation: int, n: int, n_ctx: int,
                        cap_new: int, d_kind: int, d_ctx_out: int, d_status_out: int, d_n_proposed: int,
                        ctx_base: int = 0, d_new_ctx: Optional[int] = None, d_direction: Optional[int] = None,
                        d_ttl: Optional[int] = None, d_new_placement: Optional[int] = None, terminating: bool = False,
                        d_new_idx: Optional[int] = None, d_n_new: Optional[int] = None,
                        d_gone_idx: Optional[int] = None, d_n_gone: Optional[int] = None,
                        d_target_grain: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_activate_device(self.h, V(d_ctx), V(d_recv_status), V(d_target_grain), V(d_target_activation),
                                       V(d_direction), V(d_ttl), V(d_new_placement), n, n_ctx, int(terminating),
                                       ctx_base, V(d_new_ctx), cap_new, V(d_kind), V(d_ctx_out), V(d_status_out),
                                       V(d_new_idx), V(d_n_new), V(d_gone_idx), V(d_n_gone), V(d_n_proposed)))

    @staticmethod
    def activate_io_device(cap_new: int, d_kind: int, d_n_proposed: int, ctx_base: int = 0,
                           d_new_ctx: Optional[int] = None, d_new_placement: Optional[int] = None,
                           terminating: bool = False, d_new_idx: Optional[int] = None, d_n_new: Optional[int] = None,
                           d_gone_idx: Optional[int] = None, d_n_gone: Optional[int] = None) -> gd_activate_io:
        return gd_activate_io(d_new_placement or None, int(terminating), ctx_base, d_new_ctx or None, cap_new,
                              d_kind or None, d_new_idx or None, d_n_new or None, d_gone_idx or None, d_n_gone or None,
                              d_n_proposed or None)

    def _activate_io_host(self, n, cap_new, ctx_base, new_ctx, new_placement, terminating):
        """(gd_activate_io with host pointers, result(), the arrays kept alive)."""
        npl, nc = self._opt(new_placement, np.uint8), self._opt(new_ctx, np.uint32)
        kind = np.zeros(n, np.uint8)
        new_idx, gone_idx = np.zeros(max(n, 1), np.uint32), np.zeros(max(n, 1), np.uint32)
        words = np.zeros(3, np.uint32)
        p = lambda a: None if a is None else _ptr(a)
        w = lambda k: words.ctypes.data + 4 * k
        io = gd_activate_io(p(npl), int(terminating), ctx_base, p(nc), cap_new, _ptr(kind), _ptr(new_idx), w(0),
                            _ptr(gone_idx), w(1), w(2))
        result = lambda: dict(kind=kind, new_idx=new_idx[:int(words[0])].copy(),
                              gone_idx=gone_idx[:int(words[1])].copy(), n_proposed=int(words[2]))
        return io, result, (npl, nc, kind, new_idx, gone_idx, words)

    def receive_activate_turns(self, target_grain, target_activation, n_ctx: int, ctx_flags, num_running,
                               request_count, cap_new: int, ctx_base: int = 0, new_ctx=None, new_placement=None,
                               terminating: bool = False, direction=None, ttl=None, forward_count=None, msg_flags=None,
                               sending_activation=None, hard_limit: int = 0, hard_limit_sw: int = 0,
                               max_forward_count: int = 2, chain: bool = False) -> dict:
        """gd_receive_activate_turns: activate()'s dict (ctx / status resolved) plus perm, offsets[n_ctx + 3], turn,
        num_running_out, running_idx, start_idx, wait_perm, wait_offsets[n_ctx + 2]."""
        tg, ta = keys_array(target_grain), keys_array(target_activation)
        n = len(tg)
        sa = None if sending_activation is None else keys_array(sending_activation)
        dr, tl = self._opt(direction, np.uint8), self._opt(ttl, np.int64)
        fw, mf = self._opt(forward_count, np.uint8), self._opt(msg_flags, np.uint8)
        fl, nr = self._opt(ctx_flags, np.uint8), self._opt(num_running, np.uint32)
        rc = self._opt(request_count, np.uint32)
        p = lambda a: None if a is None else _ptr(a)
        st = gd_turn_state(p(fl), p(nr), p(rc), hard_limit, hard_limit_sw, max_forward_count, int(chain))
        ctx, rst = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        perm, offs = np.zeros(n, np.uint32), np.zeros(n_ctx + 3, np.uint32)
        turn, nro, run = np.zeros(n, np.uint8), np.zeros(n_ctx, np.uint32), np.zeros(n_ctx, np.uint32)
        start, n_start = np.zeros(max(n, 1), np.uint32), np.zeros(1, np.uint32)
        wperm, woff = np.zeros(n, np.uint32), np.zeros(n_ctx + 2, np.uint32)
        io, result, keep = self._activate_io_host(n, cap_new, ctx_base, new_ctx, new_placement, terminating)

        def full():
            return dict(result(), ctx=ctx, status=rst, perm=perm, offsets=offs, turn=turn, num_running_out=nro,
                        running_idx=run, start_idx=start[:int(n_start[0])].copy(), wait_perm=wperm, wait_offsets=woff)
        try:
            self._c(lib.gd_receive_activate_turns(self.h, _ptr(tg), _ptr(ta), p(dr), n, n_ctx, None, _ptr(ctx),
                                                  _ptr(rst), _ptr(perm), _ptr(offs), p(tl), p(fw), p(mf), p(sa),
                                                  C.byref(st), _ptr(turn), _ptr(nro), _ptr(run), _ptr(start),
                                                  _ptr(n_start), _ptr(wperm), _ptr(woff), C.byref(io)))
        except GrainDispatchError as ex:
            ex.arrays = full()
            raise
        return full()

    def receive_activate_turns_device(self, d_tg: int, d_ta: int, d_dir: Optional[int], n: int, n_ctx: int, d_ctx: int,
                                      d_status: int, d_perm: Optional[int], d_offsets: Optional[int],
                                      d_ttl: Optional[int], d_forward_count: Optional[int], d_msg_flags: Optional[int],
                                      d_sending_activation: Optional[int], state: gd_turn_state, d_turn: int,
                                      d_num_running_out: int, d_running_idx: int, act: gd_activate_io,
                                      d_start_idx: Optional[int] = None, d_n_start: Optional[int] = None,
                                      d_wait_perm: Optional[int] = None, d_wait_offsets: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_receive_activate_turns_device(
            self.h, V(d_tg), V(d_ta), V(d_dir), n, n_ctx, None, V(d_ctx), V(d_status), V(d_perm), V(d_offsets), V(d_ttl),
            V(d_forward_count), V(d_msg_flags), V(d_sending_activation), C.byref(state), V(d_turn), V(d_num_running_out),
            V(d_running_idx), V(d_start_idx), V(d_n_start), V(d_wait_perm), V(d_wait_offsets), C.byref(act)))

    def receive_activate_turns_frames(self, buf: bytes, offsets, n_ctx: int, ctx_flags, num_running, request_count,
                                      cap_new: int, ctx_base: int = 0, new_ctx=None, terminating: bool = False,
                                      ttl_age_ticks: int = 0, msg_flags_or=None, hard_limit: int = 0,
                                      hard_limit_sw: int = 0, max_forward_count: int = 2, chain: bool = False) -> dict:
        """gd_receive_activate_turns_frames: receive_activate_turns()'s dict, fed from the receive buffer."""
        b = np.frombuffer(buf, dtype=np.uint8) if len(buf) else np.zeros(1, dtype=np.uint8)
        off = np.ascontiguousarray(np.asarray(offsets, dtype=np.uint64))
        n = len(off)
        mor = self._opt(msg_flags_or, np.uint8)
        fl, nr = self._opt(ctx_flags, np.uint8), self._opt(num_running, np.uint32)
        rc = self._opt(request_count, np.uint32)
        p = lambda a: None if a is None else _ptr(a)
        st = gd_turn_state(p(fl), p(nr), p(rc), hard_limit, hard_limit_sw, max_forward_count, int(chain))
        ctx, rst = np.zeros(n, np.uint32), np.zeros(n, np.uint8)
        perm, offs = np.zeros(n, np.uint32), np.zeros(n_ctx + 3, np.uint32)
        turn, nro, run = np.zeros(n, np.uint8), np.zeros(n_ctx, np.uint32), np.zeros(n_ctx, np.uint32)
        start, n_start = np.zeros(max(n, 1), np.uint32), np.zeros(1, np.uint32)
        wperm, woff = np.zeros(n, np.uint32), np.zeros(n_ctx + 2, np.uint32)
        io, result, keep = self._activate_io_host(n, cap_new, ctx_base, new_ctx, None, terminating)

        def full():
            return dict(result(), ctx=ctx, status=rst, perm=perm, offsets=offs, turn=turn, num_running_out=nro,
                        running_idx=run, start_idx=start[:int(n_start[0])].copy(), wait_perm=wperm, wait_offsets=woff)
        try:
            self._c(lib.gd_receive_activate_turns_frames(
                self.h, _ptr(b), len(buf), _ptr(off), n, n_ctx, None, None, None, _ptr(ctx), _ptr(rst), _ptr(perm),
                _ptr(offs), ttl_age_ticks, p(mor), C.byref(st), _ptr(turn), _ptr(nro), _ptr(run), _ptr(start),
                _ptr(n_start), _ptr(wperm), _ptr(woff), C.byref(io)))
        except GrainDispatchError as ex:
            ex.arrays = full()
            raise
        return full()

    def receive_activate_turns_frames_device(self, d_buf: int, buf_len: int, d_offsets: int, n: int, n_ctx: int,
                                             d_ctx: int, d_status: int, d_perm: Optional[int], d_offs: Optional[int],
                                             ttl_age_ticks: int, d_msg_flags_or: Optional[int], state: gd_turn_state,
                                             d_turn: int, d_num_running_out: int, d_running_idx: int,
                                             act: gd_activate_io, d_start_idx: Optional[int] = None,
                                             d_n_start: Optional[int] = None, d_wait_perm: Optional[int] = None,
                                             d_wait_offsets: Optional[int] = None):
        V = lambda x: C.c_void_p(x or 0)
        self._c(lib.gd_receive_activate_turns_frames_device(
            self.h, V(d_buf), buf_len, V(d_offsets), n, n_ctx, None, None, None, V(d_ctx), V(d_status), V(d_perm),
            V(d_offs), ttl_age_ticks, V(d_msg_flags_or), C.byref(state), V(d_turn), V(d_num_running_out),
            V(d_running_idx), V(d_start_idx), V(d_n_start), V(d_wait_perm), V(d_wait_offsets), C.byref(act)))

    # -- per-kernel timing ----------------------------------------------------------
    def kernel_times(self) -> dict:
        arr = (gd_kernel_time * 64)()
        n = C.c_uint32(0)
        self._c(lib.gd_kernel_times(self.h, arr, 64, C.byref(n)))
        return {arr[i].name.decode(): (int(arr[i].launches), float(arr[i].total_ms)) for i in range(min(n.value, 64))}

    def set_kernel_timing(self, enable):
        """False / True: off / every launch; 2: the stages only ("stage:bucket")."""
        self._c(lib.gd_set_kernel_timing(self.h, 2 if enable == 2 else (1 if enable else 0)))

    def kernel_times_reset(self):
        self._c(lib.gd_kernel_times_reset(self.h))


class MicroBatch:
    """gd_microbatch: pinned host buffers + a hipGraph per batch size.
    `keys`, `silo`, `act`, `status`, `perm`, `run_start`, `run_act` are numpy views of the
    pinned buffers (no copies); `n_runs` reads the run count of the last run()."""

    def __init__(self, dispatch: GrainDispatch, capacity: int, n_act: int):
        self.gd = dispatch
        self.capacity, self.n_act = capacity, n_act
        mb = C.c_void_p()
        _check(dispatch.h, lib.gd_microbatch_create(dispatch.h, capacity, n_act, C.byref(mb)))
        self.mb = mb
        kp = lib.gd_microbatch_keys(mb)
        self.keys = np.ctypeslib.as_array(C.cast(kp, C.POINTER(C.c_uint64)), shape=(capacity, 3))
        ptrs = [C.c_void_p() for _ in range(7)]
        _check(dispatch.h, lib.gd_microbatch_outputs(mb, *[C.byref(x) for x in ptrs]))
        u32 = lambda p, n: np.ctypeslib.as_array(C.cast(p, C.POINTER(C.c_uint32)), shape=(n,))
        self.silo = u32(ptrs[0], capacity)
        self.act = u32(ptrs[1], capacity)
        self.status = np.ctypeslib.as_array(C.cast(ptrs[2], C.POINTER(C.c_uint8)), shape=(capacity,))
        self.perm = u32(ptrs[3], capacity)
        self._n_runs = u32(ptrs[4], 1)
        self.run_start = u32(ptrs[5], capacity + 1)
        self.run_act = u32(ptrs[6], capacity)

    @property
    def n_runs(self) -> int:
        return int(self._n_runs[0])

    def offsets(self) -> np.ndarray:
        """The runs expanded to gd_bucket's offsets[n_act + 2] (for comparison with it)."""
        r = self.n_runs
        out = np.empty(self.n_act + 2, dtype=np.uint32)
        # offsets[a] = start of the first run with activation >= a; empty buckets share it
        starts = np.append(self.run_start[:r], self.run_start[r])
        acts = np.append(self.run_act[:r].astype(np.int64), self.n_act + 1)
        idx = np.searchsorted(acts, np.arange(self.n_act + 2), side="left")
        out[:] = starts[idx]
        return out

    def run(self, n: int, use_graph: bool = True):
        _check(self.gd.h, lib.gd_microbatch_run(self.mb, n, 1 if use_graph else 0))

    def close(self):
        if getattr(self, "mb", None):
            lib.gd_microbatch_destroy(self.mb)
            self.mb = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
