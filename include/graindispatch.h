/*
 * graindispatch.h -- C ABI of libgraindispatch.so, the MI355X (gfx950) batched
 * message-routing engine for the Orleans virtual-actor dispatch path.
 *
 * The Orleans host (C#) keeps its Dispatcher / MessageCenter / IGrainFactory
 * surface.  A batching stage hands message headers to this library through
 * P/Invoke (see INTEGRATION.md for the [DllImport] stubs).  Plain pointers and
 * sizes only; no exceptions cross this boundary; every entry point returns
 * GD_OK (0) or a negative GD_E* code, with a message in gd_last_error().
 *
 * Reference interfaces each entry point replaces (paths relative to the
 * rikbosch/orleans root):
 *   ring       LocalGrainDirectory.CalculateTargetSilo      src/Orleans.Runtime/GrainDirectory/LocalGrainDirectory.cs:477-545
 *              IConsistentRingProvider.GetPrimaryTargetSilo src/Orleans.Runtime/ConsistentRing/IConsistentRingProvider.cs:34
 *              (ConsistentRingProvider.cs:322-372, VirtualBucketsRingProvider.cs:244-293)
 *              ring rebuild: LocalGrainDirectory.AddServer  LocalGrainDirectory.cs:284-309,
 *              VirtualBucketsRingProvider.AddServer         VirtualBucketsRingProvider.cs:122-149
 *   directory  GrainDirectoryPartition.AddSingleActivation  src/Orleans.Runtime/GrainDirectory/GrainDirectoryPartition.cs:304-326
 *              GrainDirectoryPartition.RemoveActivation     GrainDirectoryPartition.cs:335-363
 *              GrainDirectoryPartition.LookUpActivations    GrainDirectoryPartition.cs:385-441
 *              ILocalGrainDirectory.LocalLookup             src/Orleans.Runtime/GrainDirectory/ILocalGrainDirectory.cs:22
 *   address    Dispatcher.AddressMessage                    src/Orleans.Runtime/Core/Dispatcher.cs:715-767
 *   enqueue    IncomingMessageAgent.ReceiveMessage          src/Orleans.Runtime/Messaging/IncomingMessageAgent.cs:92-190
 *              + ActivationData.EnqueueMessage (FIFO)       src/Orleans.Runtime/Catalog/ActivationData.cs:566-606
 *   identity   JenkinsHash.ComputeHash                      src/Orleans.Core.Abstractions/IDs/JenkinsHash.cs:25-105
 *              UniqueKey.GetUniformHashCode                 src/Orleans.Core.Abstractions/IDs/UniqueKey.cs:272-293
 *              SiloAddress.GetConsistentHashCode / GetUniformHashCodes  SiloAddress.cs:164-248
 *              Utils.CalculateIdHash                        src/Orleans.Core/Utils/Utils.cs:184-203
 *
 * Threading: one handle = one HIP stream.  Calls on a handle are serialised
 * by the caller (the reference serialises the same state under
 * lock(membershipCache) / lock(lockable), LocalGrainDirectory.cs:512,
 * GrainDirectoryPartition.cs:282,393).  gd_ring_set installs a new immutable
 * ring snapshot that the next route call uses (the mirror of the lock-free
 * snapshot swap at VirtualBucketsRingProvider.cs:143-144).
 *
 * Ownership: host arrays are caller-owned and never retained past return.
 * *_device entry points take device pointers (hipMalloc'd / torch tensors)
 * and only enqueue on the handle's stream; call gd_synchronize() before
 * reading results.  The library owns the table, ring snapshot and scratch.
 */
#ifndef GRAINDISPATCH_H
#define GRAINDISPATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GD_ABI_VERSION 1

/* ---- return codes ------------------------------------------------------ */
#define GD_OK        0
#define GD_EINVAL   -1   /* bad argument / unsorted ring / n too large       */
#define GD_ENOMEM   -2   /* device or host allocation failed                 */
#define GD_EHIP     -3   /* HIP runtime error                                */
#define GD_ERCCL    -4   /* collective error (multi-GPU path)                */
#define GD_EFULL    -5   /* directory table cannot take more entries         */
#define GD_ESTATE   -6   /* no ring installed / handle not ready             */
#define GD_ETIMEOUT -7   /* a bounded device spin gave up (never expected)   */

/* ---- ring modes ----------------------------------------- */
#define GD_RING_DIRECTORY        0 /* D: LocalGrainDirectory, signed predecessor, wrap to last */
#define GD_RING_CONSISTENT       1 /* R: ConsistentRingProvider, (long)int >= (long)uint, wrap to first */
#define GD_RING_VIRTUAL_BUCKETS  2 /* V: VirtualBucketsRingProvider, uint successor, wrap to first */

/* ---- per-message routing status (out_status) ------------------------------ */
#define GD_ROUTE_OK             0 /* directory hit: (silo, act) = the single activation     */
#define GD_ROUTE_MISS           1 /* not registered: C# slow path (Dispatcher.cs:742);
                                     out_silo = directory owner silo                         */
#define GD_ROUTE_SYSTEM_TARGET  2 /* UniqueKey category SystemTarget: out_silo = my silo
                                     (LocalGrainDirectory.cs:480-485)                         */
#define GD_ROUTE_MEMBERSHIP     3 /* Constants.SystemMembershipTableId: out_silo = seed silo
                                     (LocalGrainDirectory.cs:487-503)                         */
#define GD_ROUTE_KEYEXT         4 /* KeyExtGrain / GeoClient: the uniform hash needs the
                                     KeyExt string (UniqueKey.cs:279-281); C# handles it     */

#define GD_ROUTE_MULTI_ACT      7 /* the grain has several activations (GrainInfo.Instances.Count >= 2,
                                     e.g. StatelessWorker): RandomPlacementDirector picks one in C#
                                     (RandomPlacementDirector.cs:33-53); out_silo = directory owner.
                                     A StatelessWorker class's own messages: gd_workers_select* */

#define GD_NO_ACTIVATION 0xFFFFFFFFu
#define GD_ACT_MULTI     0xFFFFFFFEu   /* gd_val.act of a multi-activation grain (gd_dir_upsert)   */
#define GD_NO_SILO       0xFFFFFFFFu

/* UniqueKey fields (UniqueKey.cs:28-31) of a GrainId.  24 bytes, AoS. */
typedef struct gd_key {
    uint64_t n0;
    uint64_t n1;
    uint64_t type_code_data;
} gd_key;

/* Directory value: the compact form of ActivationAddress (ActivationAddress.cs:6-34).
 * act  = host-side activation index (the C# side maps it to its ActivationData),
 * silo = index into the host's silo table. */
typedef struct gd_val {
    uint32_t act;
    uint32_t silo;
} gd_val;

/* SiloAddress (SiloAddress.cs:33-35): IPv4 in ip[12..15] with is_v4 = 1
 * (BinaryTokenStreamWriter.cs:485-500 layout), or 16-byte IPv6. */
typedef struct gd_silo_addr {
    uint8_t ip[16];
    int32_t port;
    int32_t generation;
    int32_t is_v4;
} gd_silo_addr;

typedef struct gd_config {
    uint32_t struct_size;     /* sizeof(gd_config)                                   */
    int32_t  device;          /* HIP device ordinal                                  */
    uint64_t table_capacity;  /* directory slots (rounded up to a power of two);
                                 0 = 1<<20.  Keep load <= 0.5 for short probes.      */
    uint32_t my_silo;         /* silo index this handle acts for (system targets)    */
    uint32_t seed_silo;       /* owner of the membership-table grain; GD_NO_SILO = none */
    uint32_t max_batch;       /* messages per call the scratch is sized for (0 = 1<<24);
                                 larger calls grow the scratch (outside graph capture) */
    uint32_t flags;           /* GD_CFG_* bits                                       */
} gd_config;

#define GD_CFG_KERNEL_TIMING 1u  /* record per-kernel HIP events (gd_kernel_times) */
#define GD_CFG_NO_LANE_ORDER 2u  /* behave as on a device whose LDS atomics are not served in lane order:
                                    every stable rank by ballots (GD_OPT_STABLE_RANK 0, 1 refused); the
                                    library's own choice when gd_create's check fails (tests force it) */

typedef struct gd_stats {
    uint64_t routed;          /* messages through gd_route*                          */
    uint64_t table_live;      /* live directory entries                              */
    uint64_t table_tombstones;
    uint64_t table_capacity;
    uint64_t ring_points;
    uint64_t ring_mode;
} gd_stats;

typedef struct gd_handle gd_handle;

/* ---- lifecycle -------------------------------------------------------------- */
int         gd_create(const gd_config* cfg, gd_handle** out);
void        gd_destroy(gd_handle* h);
const char* gd_last_error(const gd_handle* h);   /* never NULL; h may be NULL     */
int         gd_abi_version(void);
int         gd_set_stream(gd_handle* h, void* hip_stream); /* NULL = library stream */
void*       gd_get_stream(gd_handle* h);
/* Pinned (page-locked) host memory for batch buffers.  The host-pointer entry points overlap
 * their PCIe copies with the kernels for large batches (gd_route_bucket: keys up, routes down
 * while later chunks are probed); the copies are asynchronous only from pinned memory.  A C# host
 * allocates its batch arrays here once and reuses them (Span<T> over the pointer). */
int         gd_host_alloc(size_t bytes, void** out);
int         gd_host_free(void* p);
int         gd_synchronize(gd_handle* h);
int         gd_stats_get(gd_handle* h, gd_stats* out);

/* ---- identity (host; L0) ------------------------------------------------------ */
uint32_t gd_jenkins_hash_bytes(const uint8_t* data, size_t len);                 /* JenkinsHash.cs:25-74  */
uint32_t gd_jenkins_hash_u64x3(uint64_t u1, uint64_t u2, uint64_t u3);          /* JenkinsHash.cs:85-105 */
uint32_t gd_uniform_hash(const gd_key* key);                                     /* UniqueKey.cs:272-293 (no KeyExt) */
int32_t  gd_calculate_id_hash(const char* utf8_text);                            /* Utils.cs:184-203      */
int32_t  gd_silo_consistent_hash(const gd_silo_addr* silo);                      /* SiloAddress.cs:164-173 */
int      gd_silo_uniform_hashes(const gd_silo_addr* silo, uint32_t n, uint32_t* out); /* SiloAddress.cs:197-248 */
int      gd_silo_compare(const gd_silo_addr* a, const gd_silo_addr* b);          /* SiloAddress.cs:280-329 */

/* ---- ring ------------------------------------------------------------------- */
/* Build a ring from silos added in the given order (membership-change order):
 * mode D/R -> AddServer sorted insert by signed consistent hash (ties: newcomer
 * before equals); mode V -> buckets_per_silo uniform points per silo, uint
 * sorted, collision -> lesser SiloAddress.  out_points / out_owner must hold
 * n_silos (D/R) or n_silos*buckets_per_silo (V) entries; *out_n = ring size. */
int gd_ring_build(int mode, const gd_silo_addr* silos, uint32_t n_silos, uint32_t buckets_per_silo,
                  uint32_t* out_points, uint32_t* out_owner, uint32_t* out_n);
/* Install a ring snapshot: points are 32-bit patterns in ring order (int32 sorted
 * ascending for D/R, uint32 ascending for V); owner[i] = silo index of point i. */
int gd_ring_set(gd_handle* h, int mode, const uint32_t* points, const uint32_t* owner, uint32_t n);

/* CalculateTargetSilo(GrainId) for a batch: directory-owner silo per key
 * (special categories follow the same rules as gd_route).  Host pointers. */
int gd_ring_owner(gd_handle* h, const gd_key* keys, uint32_t n, uint32_t* out_silo);
/* GetPrimaryTargetSilo(uint key) for a batch of raw ring keys.  Host pointers. */
int gd_ring_lookup_hashes(gd_handle* h, const uint32_t* hashes, uint32_t n, uint32_t* out_silo);

/* ---- directory (one table per handle = the silo partitions this GPU owns) ---- */
/* AddSingleActivation for a batch, applied in batch order: the first registration
 * of a grain wins; out_vals receives the winning (act, silo) for every item and
 * out_inserted 1 for the item that created the entry.  Host pointers. */
int gd_dir_register(gd_handle* h, const gd_key* keys, const gd_val* vals, uint32_t n,
                    gd_val* out_vals, uint8_t* out_inserted);
/* gd_dir_register with device arrays (keys, values and the optional outputs, which may be NULL):
 * bulk population of a partition whose grains are already in HBM (activation tables built on
 * the GPU, a handoff received over RCCL).  Waits for work enqueued on the handle's stream, runs
 * synchronously.  A value with silo > 0xFFFE fails the call with GD_EINVAL. */
int gd_dir_register_device(gd_handle* h, const gd_key* d_keys, const gd_val* d_vals, uint32_t n,
                           gd_val* d_out_vals, uint8_t* d_out_inserted);
/* Overwrite for a batch, applied in batch order (the last item of a grain wins): how the host
 * mirrors GrainDirectoryPartition.AddActivation (GrainDirectoryPartition.cs:274-302; GrainInfo
 * .AddActivation :89-108) for multi-instance grains: one instance -> {act, silo}, two or more ->
 * {GD_ACT_MULTI, any silo} (routes then return GD_ROUTE_MULTI_ACT).  out_inserted[i] = 1 for the
 * item that created a grain's entry (may be NULL).  Host pointers. */
int gd_dir_upsert(gd_handle* h, const gd_key* keys, const gd_val* vals, uint32_t n, uint8_t* out_inserted);
/* RemoveActivation(grain, act) for a batch; out_removed may be NULL. */
int gd_dir_unregister(gd_handle* h, const gd_key* keys, const uint32_t* acts, uint32_t n,
                      uint8_t* out_removed);
/* The continuous-registration forms (round 6): activations register and deactivate all the time
 * (Catalog.cs:540-552,1270-1277 -> GrainDirectoryPartition.AddSingleActivation / RemoveActivation,
 * GrainDirectoryPartition.cs:304-363), between route batches.  Both only enqueue on the handle's
 * stream (device arrays, outputs optional): no host round trip, so a host interleaves them with
 * gd_route_bucket_device batches and the stream runs them back to back; the probe indexes are
 * re-projected for the touched slots, not rebuilt.  Same semantics as gd_dir_register_device /
 * gd_dir_unregister; a device-side failure (table full, a silo index above 0xFFFE: GD_EINVAL, claims
 * not settled after the gated passes) is returned once by the next synchronising call on the handle
 * (gd_synchronize, gd_stats_get, ...); a synchronous gd_dir_register / gd_dir_register_device that
 * comes first returns it before doing any work of its own, and succeeds when repeated.
 * gd_dir_unregister_device with d_out_removed NULL is one launch (which of a key's matching items
 * removes it is then unobservable: the CAS on the entry's LIVE meta picks it); with a report, the
 * first matching item of the batch is elected in a second launch. */
int gd_dir_register_device_async(gd_handle* h, const gd_key* d_keys, const gd_val* d_vals, uint32_t n,
                                 gd_val* d_out_vals, uint8_t* d_out_inserted);
int gd_dir_unregister_device(gd_handle* h, const gd_key* d_keys, const uint32_t* d_acts, uint32_t n,
                             uint8_t* d_out_removed);
/* LookUpActivations for a batch; out_found[i] = 0 -> out_vals[i] = {GD_NO_ACTIVATION, GD_NO_SILO}. */
int gd_dir_lookup(gd_handle* h, const gd_key* keys, uint32_t n, gd_val* out_vals, uint8_t* out_found);
int gd_dir_clear(gd_handle* h);
/* Rebuild into a table of new_capacity slots (drops tombstones). */
int gd_dir_rehash(gd_handle* h, uint64_t new_capacity);

/* ---- KeyExt grains (string keys, compound keys, geo clients) ---------
 * UniqueKey.HasKeyExt categories (KeyExtGrain 6, GeoClient 7; UniqueKey.cs:60-66) hash
 * JenkinsHash.ComputeHash(ToByteArray()) = N0|N1|TCD|int32 len|UTF-8 when KeyExt != null
 * (UniqueKey.cs:272-336) and compare the KeyExt string (UniqueKey.cs:245-251).  They live in a
 * second table (64-B slots + a KeyExt byte heap).  A batch's KeyExt strings travel beside the
 * 24-B keys: message i's UTF-8 bytes are bytes[offset[i] .. offset[i] + length[i]).  Messages
 * of other categories ignore their entry.  Equality is on UTF-8 bytes, which is C#'s ordinal
 * equality except for strings with unpaired surrogates (Encoding.UTF8 maps them to U+FFFD):
 * send those as GD_KEYEXT_HOST and they keep status GD_ROUTE_KEYEXT. */
#define GD_KEYEXT_NULL (-1)   /* KeyExt == null: three-word hash; equal only to a null KeyExt */
#define GD_KEYEXT_HOST (-2)   /* leave the message to the C# path (status GD_ROUTE_KEYEXT)    */
typedef struct gd_key_ext {
    const uint8_t*  bytes;      /* UTF-8 KeyExt strings of the batch, concatenated      */
    const uint64_t* offset;     /* [n] start of message i's string in bytes              */
    const int32_t*  length;     /* [n] UTF-8 byte length, GD_KEYEXT_NULL or GD_KEYEXT_HOST */
    uint64_t        bytes_len;  /* size of bytes (offset + length beyond it -> KEYEXT)  */
} gd_key_ext;

/* AddSingleActivation / RemoveActivation / LookUpActivations for KeyExt grains, batch order,
 * first registration wins (as gd_dir_register).  Keys must have a KeyExt category (GD_EINVAL
 * otherwise).  Registrations are applied to a host-side index of the table and the changed
 * slots uploaded (registration is off the per-message path); lookups run on the GPU.
 * Host pointers (ext included). */
int gd_dir_register_ext(gd_handle* h, const gd_key* keys, const gd_key_ext* ext, const gd_val* vals, uint32_t n,
                        gd_val* out_vals, uint8_t* out_inserted);
int gd_dir_unregister_ext(gd_handle* h, const gd_key* keys, const gd_key_ext* ext, const uint32_t* acts,
                          uint32_t n, uint8_t* out_removed);
int gd_dir_lookup_ext(gd_handle* h, const gd_key* keys, const gd_key_ext* ext, uint32_t n, gd_val* out_vals,
                      uint8_t* out_found);
/* UniqueKey.GetUniformHashCode of KeyExt keys computed on the device (the hash k_route_keyext
 * uses; 0 for GD_KEYEXT_HOST items).  Host pointers. */
int gd_uniform_hashes_ext(gd_handle* h, const gd_key* keys, const gd_key_ext* ext, uint32_t n, uint32_t* out);
/* KeyExt entries, capacity, heap bytes in use. */
int gd_dir_ext_stats(gd_handle* h, uint64_t* live, uint64_t* capacity, uint64_t* heap_bytes);

/* gd_route / gd_route_bucket with KeyExt grains routed on the GPU too (their status is then
 * OK or MISS like any grain; GD_KEYEXT_HOST items stay GD_ROUTE_KEYEXT).  ext == NULL behaves
 * as gd_route.  Host pointers. */
int gd_route_ext(gd_handle* h, const gd_key* keys, const gd_key_ext* ext, uint32_t n,
                 uint32_t* out_silo, uint32_t* out_act, uint8_t* out_status);
int gd_route_bucket_ext(gd_handle* h, const gd_key* keys, const gd_key_ext* ext, uint32_t n, uint32_t n_act,
                        uint32_t* out_silo, uint32_t* out_act, uint8_t* out_status,
                        uint32_t* out_perm, uint32_t* out_offsets);
/* Device forms: d_keys and the arrays inside *d_ext are device pointers (d_ext itself is a host
 * struct).  Enqueue only. */
int gd_route_ext_device(gd_handle* h, const gd_key* d_keys, const gd_key_ext* d_ext, uint32_t n,
                        uint32_t* d_silo, uint32_t* d_act, uint8_t* d_status);
int gd_route_bucket_ext_device(gd_handle* h, const gd_key* d_keys, const gd_key_ext* d_ext, uint32_t n,
                               uint32_t n_act, uint32_t* d_silo, uint32_t* d_act, uint8_t* d_status,
                               uint32_t* d_perm, uint32_t* d_offsets);

/* ---- the hot path -------------------------------------------------------------- */
/* Address a batch: ring lookup + directory probe.  Host pointers. */
int gd_route(gd_handle* h, const gd_key* keys, uint32_t n,
             uint32_t* out_silo, uint32_t* out_act, uint8_t* out_status);
/* Per-activation bucketing: stable partition of message indices by activation.
 * acts >= n_act (e.g. GD_NO_ACTIVATION) go to the trailing bucket n_act.
 * out_perm[n]; out_offsets[n_act + 2] (bucket a = [off[a], off[a+1])).  Host pointers. */
int gd_bucket(gd_handle* h, const uint32_t* acts, uint32_t n, uint32_t n_act,
              uint32_t* out_perm, uint32_t* out_offsets);
/* Fused route + bucket.  Host pointers. */
int gd_route_bucket(gd_handle* h, const gd_key* keys, uint32_t n, uint32_t n_act,
                    uint32_t* out_silo, uint32_t* out_act, uint8_t* out_status,
                    uint32_t* out_perm, uint32_t* out_offsets);

/* Device-pointer forms (enqueue only).  Same semantics as above.  One exception to "enqueue only": the
 * first large route after a directory change the probe indexes do not track (rehash, clear, silo
 * removal, merge, split, handoff; gd_index_stats below) rebuilds them (two streaming passes over the
 * table) and synchronises the handle's stream once to read the build's counters;
 * registration / upsert / unregister batches keep the indexes current and routes after them enqueue
 * only.  gd_option_set(GD_OPT_PROBE, 0) turns the indexes off. */
int gd_route_device(gd_handle* h, const gd_key* d_keys, uint32_t n,
                    uint32_t* d_silo, uint32_t* d_act, uint8_t* d_status);
int gd_bucket_device(gd_handle* h, const uint32_t* d_acts, uint32_t n, uint32_t n_act,
                     uint32_t* d_perm, uint32_t* d_offsets);
int gd_route_bucket_device(gd_handle* h, const gd_key* d_keys, uint32_t n, uint32_t n_act,
                           uint32_t* d_silo, uint32_t* d_act, uint8_t* d_status,
                           uint32_t* d_perm, uint32_t* d_offsets);
/* Pipelining of batches (no reference counterpart): with a bucket stream set (non-NULL, not the handle's
 * stream), gd_route_bucket_device enqueues the route on the handle's stream and the bucketing on the
 * bucket stream after it (an event), without making the handle's stream wait: the next batch's route
 * overlaps this batch's bucketing.  The caller must not reuse a batch's act / perm / offsets before the
 * bucket stream has passed them (an event on it, or gd_synchronize, which waits for both streams).
 * NULL restores the default (everything on the handle's stream).  Synchronizes the handle.
 * Measured on MI355X (profiles/r05_pipeline_ab.txt): route and bucketing contend for HBM and L2, and the
 * overlap is slower than the serial order (BASELINE cfg 2 -4 %, cfg 3 -30 %); off by default. */
int gd_set_bucket_stream(gd_handle* h, void* hip_stream);
int gd_ring_owner_device(gd_handle* h, const gd_key* d_keys, uint32_t n, uint32_t* d_silo);

/* ---- multi-GPU helpers (directory sharded by ring owner, SURVEY 8 e) ------------ */
/* Stable partition of a batch by destination shard = owner_silo % n_shards
 * (owner from the installed ring).  Writes the keys in shard order to
 * d_send_keys, the original message index to d_send_idx, and per-shard
 * message counts to d_counts[n_shards].  Device pointers; n_shards <= 256. */
int gd_pack_by_shard_device(gd_handle* h, const gd_key* d_keys, uint32_t n, uint32_t n_shards,
                            gd_key* d_send_keys, uint32_t* d_send_idx, uint32_t* d_counts);
/* The second hop when the directory owner is not the activation's silo (ActivationAddress.Silo,
 * the send after a remote lookup, LocalGrainDirectory.cs:920 -> OutboundMessageQueue.cs:125):
 * stable partition of routed messages by the rank hosting their activation -- status
 * GD_ROUTE_OK: d_silo[i] % n_shards; any other status: my_rank (the message stays on the owner).
 * Writes the keys in rank order to d_send_keys, each message's input position to d_send_pos and
 * per-rank counts to d_counts[n_shards].  Device pointers; n_shards <= 256. */
int gd_pack_routes_by_rank_device(gd_handle* h, const gd_key* d_keys, const uint8_t* d_status,
                                  const uint32_t* d_silo, uint32_t n, uint32_t n_shards, uint32_t my_rank,
                                  gd_key* d_send_keys, uint32_t* d_send_pos, uint32_t* d_counts);

/* ---- in-library exchange over RCCL (SURVEY 8 b gd_route_multi, 8 e) ------------------
 * One process (one handle) per GPU.  Rank r hosts the directory partitions of silos
 * s with s % n_ranks == r (GrainDirectoryPartition per silo, LocalGrainDirectory.cs:477-545).
 * gd_route_multi sends each message of a rank's batch to the rank owning its grain
 * (the per-target-silo outbound queues of OutboundMessageQueue.SendMessage,
 * OutboundMessageQueue.cs:54-131, as one grouped RCCL send/recv over xGMI), probes the
 * directory and buckets per activation there (IncomingMessageAgent.cs:92-190), and with
 * return_routes sends (silo, act, status) back so the sender holds each of its messages'
 * target address in batch order (Dispatcher.AddressMessage, Dispatcher.cs:715-767).
 * RCCL is loaded at run time (librccl.so.1); without it these return GD_ERCCL.
 * The unique id (128 B) is created by one rank and handed to the others by the host
 * (any out-of-band channel); gd_comm_init is collective over all ranks. */
#define GD_COMM_ID_BYTES 128
int gd_comm_unique_id(uint8_t out_id[GD_COMM_ID_BYTES]);
int gd_comm_init(gd_handle* h, const uint8_t id[GD_COMM_ID_BYTES], int n_ranks, int rank);
/* Rehearsal transport: hs[0..n_ranks) (handles of this process, any devices, one host thread
 * driving each) become ranks 0..n_ranks-1 of an in-process communicator whose send/recv are
 * device-to-device copies with RCCL's matching and stream-ordering rules (gd_localcomm.h).  It
 * runs the W > 1 exchange on one GPU, which RCCL refuses (one rank per device).  Each handle
 * leaves it with gd_comm_destroy / gd_destroy. */
int gd_comm_init_local(gd_handle* const* hs, int n_ranks);
int gd_comm_destroy(gd_handle* h);

/* Results of the last gd_route_multi* call on a handle: device pointers into library-owned
 * buffers, valid until the next gd_route_multi* / gd_comm_destroy / gd_destroy.  The received
 * messages are in arrival order = (sender rank, table region, sender batch order): each sender
 * groups its chunk for an owner by the eighth of the owner's directory table the grain's home slot
 * lies in (region 0 for system targets, the membership grain and KeyExt grains), so the owner's
 * probe maps one region to one XCD.  Without header compaction (GD_COMPACT_HEADERS=0) or with
 * GD_REGION_PROBE=0 on the sender, or more than 32 ranks, the order is (sender rank, sender batch
 * order).  One grain has one region, so every activation's messages are in (sender rank, sender
 * batch order) either way; perm / offsets are the stable per-activation bucketing of the arrival
 * order (offsets: n_act + 2 entries). */
typedef struct gd_multi_result {
    uint32_t        n_recv;       /* messages this rank owns in this batch            */
    uint32_t        n_act;
    const gd_key*   recv_keys;    /* [n_recv]                                         */
    const uint32_t* recv_idx;     /* [n_recv] index in the sender's batch             */
    const uint32_t* recv_src;     /* [n_recv] sender rank                             */
    const uint32_t* silo;         /* [n_recv] route results on the owner              */
    const uint32_t* act;
    const uint8_t*  status;
    const uint32_t* perm;         /* [n_recv]                                         */
    const uint32_t* offsets;      /* [n_act + 2]                                      */
    const uint32_t* ret_silo;     /* [n] in this rank's batch order (return_routes)   */
    const uint32_t* ret_act;
    const uint8_t*  ret_status;
} gd_multi_result;

/* flags: GD_MULTI_RETURN_ROUTES -- also send (silo, act, status) back to the senders (ret_*).
 *        GD_MULTI_KEYS_READY    -- d_keys are complete already (their producer was synchronised);
 *        without it the exchange waits for all work enqueued on the handle's stream, which includes
 *        the previous batch's probe + bucketing.  With it, batch i+1's partition and RCCL rounds
 *        (on the library's exchange stream) run while batch i is probed and bucketed (on the
 *        handle's stream).  Results are complete when the handle's stream reaches them
 *        (gd_synchronize, or stream order for later work); they stay valid through the next
 *        call and are overwritten by the one after (two batches in flight).
 * Blocks the host once per call, on the per-rank counts round (it sizes the receive). */
#define GD_MULTI_RETURN_ROUTES 1
#define GD_MULTI_KEYS_READY    2
/* GD_MULTI_FORWARD -- the directory owner is not the activation's silo in general (Orleans
 *        co-locates neither; ActivationAddress.Silo): after the probe on the owner, directory hits
 *        travel on to the rank hosting their activation (silo % n_ranks, a second grouped round,
 *        gd_pack_routes_by_rank_device) and are bucketed there; every other status stays on the
 *        owner.  The result then describes the messages delivered to this rank: recv_idx / recv_src
 *        still name the original sender, silo / act / status are the owner's routes, and each
 *        activation's messages keep (sender rank, sender batch order).  A second host sync (the
 *        forward counts) per call.  Combines with GD_MULTI_RETURN_ROUTES (routes go back from the
 *        owner). */
#define GD_MULTI_FORWARD       4
/* GD_MULTI_NO_KEYS -- the result's recv_keys stay unset (NULL): the receiver identifies each
 *        message by (recv_src, recv_idx).  When every received header was compact in one form
 *        (N1 alone, 4 B when all of a sender's N1s are below 2^32, else 8 B; one TypeCodeData: the
 *        batches of every sender held long-keyed grains of one type) the probe reads the N1s
 *        directly and the 24-B keys are never rebuilt.  Ignored with
 *        GD_MULTI_FORWARD (the keys move on). */
#define GD_MULTI_NO_KEYS       8
int gd_route_multi_device(gd_handle* h, const gd_key* d_keys, uint32_t n, uint32_t n_act, int flags,
                          gd_multi_result* out);
/* Host keys in (C# pinned array), copied on the exchange stream; returns with the batch done
 * (results stay on the device -> gd_multi_fetch). */
int gd_route_multi(gd_handle* h, const gd_key* keys, uint32_t n, uint32_t n_act, int flags,
                   gd_multi_result* out);
/* CalculateTargetSilo (LocalGrainDirectory.cs:477-545) with KeyExt strings: the owner silo the
 * exchange partition uses (system targets / KeyExt without a string -> my silo, the membership
 * grain -> the seed).  Host pointers. */
int gd_ring_owner_ext(gd_handle* h, const gd_key* keys, const gd_key_ext* ext, uint32_t n, uint32_t* out_silo);
/* With the batch's KeyExt strings (gd_key_ext, as gd_route_ext): KeyExt grains go to the rank
 * owning their KeyExt hash, their strings travel in a byte round after the header round, and they
 * are routed there like any grain (without ext they stay on the sender, status GD_ROUTE_KEYEXT).
 * The _device form takes device arrays inside *d_ext. */
int gd_route_multi_ext_device(gd_handle* h, const gd_key* d_keys, const gd_key_ext* d_ext, uint32_t n,
                              uint32_t n_act, int flags, gd_multi_result* out);
int gd_route_multi_ext(gd_handle* h, const gd_key* keys, const gd_key_ext* ext, uint32_t n, uint32_t n_act,
                       int flags, gd_multi_result* out);
/* Copy the last result to host arrays sized from gd_multi_result (any pointer may be NULL). */
int gd_multi_fetch(gd_handle* h, gd_key* recv_keys, uint32_t* recv_idx, uint32_t* recv_src, uint32_t* silo,
                   uint32_t* act, uint8_t* status, uint32_t* perm, uint32_t* offsets, uint32_t* ret_silo,
                   uint32_t* ret_act, uint8_t* ret_status);

/* ---- micro-batch latency path (BASELINE config 5) ----------------------
 * Small batches (e.g. 4k messages: Presence / GPSTracker traffic,
 * Samples/GPSTracker/GPSTracker.GrainImplementation/DeviceGrain.cs:18-37) pay launch
 * and copy overheads, not bandwidth.  A micro-batch owns pinned host buffers and
 * device buffers; the whole step (H2D keys -> route -> one-workgroup stable sort by
 * activation -> one D2H of every result) is captured once per batch size as a hipGraph
 * and replayed.  Instead of gd_bucket's n_act+2 offsets it returns the runs of the
 * activations present: run r = activation run_act[r] (n_act for acts >= n_act), its
 * messages perm[run_start[r] .. run_start[r+1]) in arrival order; run_start[n_runs] = n.
 * The caller writes gd_microbatch_keys(), calls gd_microbatch_run(), reads the outputs. */
#define GD_MICROBATCH_MAX 8192u
typedef struct gd_microbatch gd_microbatch;
int      gd_microbatch_create(gd_handle* h, uint32_t capacity, uint32_t n_act, gd_microbatch** out);
void     gd_microbatch_destroy(gd_microbatch* mb);
gd_key*  gd_microbatch_keys(gd_microbatch* mb);                     /* pinned, capacity entries */
/* Pinned host results, valid after gd_microbatch_run: silo/act/status/perm[capacity],
 * n_runs[1], run_start[capacity + 1], run_act[capacity]. */
int      gd_microbatch_outputs(gd_microbatch* mb, uint32_t** silo, uint32_t** act, uint8_t** status,
                               uint32_t** perm, uint32_t** n_runs, uint32_t** run_start, uint32_t** run_act);
/* Route + bucket the first n keys (n <= capacity <= GD_MICROBATCH_MAX); synchronous.
 * use_graph = 0 runs the same launches eagerly; the graph for a given n is captured on first use. */
int      gd_microbatch_run(gd_microbatch* mb, uint32_t n, int use_graph);

/* ---- batched header decode -------------------------------------------
 * Replaces, for the fields the dispatch path reads, the per-message
 * HeadersContainer.Deserializer (src/Orleans.Core/Messaging/Message.cs:1247-1356) run by
 * IncomingMessageBuffer (src/Orleans.Core/Messaging/IncomingMessageBuffer.cs) over each frame
 * [int32 headerLength][int32 bodyLength][header][body] (Message.cs:481-516).  The caller hands
 * over the receive buffer as is plus the byte offset of every frame (the receive loop already
 * knows them from the two length prefixes). */
#define GD_FRAME_HAS_TARGET     0x01u /* TargetGrain decoded                                       */
#define GD_FRAME_COMPLETE       0x02u /* TargetGrain + TargetActivation + TargetSilo bits set:
                                         TargetAddress.IsComplete -> AddressMessage skips it        */
#define GD_FRAME_FALLBACK       0x04u /* an object-serialized field precedes a field read here:
                                         CacheInvalidationHeader / RequestContext -> nothing decoded;
                                         TargetObserver -> all but TargetSilo decoded. C# decodes it */
#define GD_FRAME_MALFORMED      0x08u /* lengths run past the header or the buffer: nothing decoded  */
#define GD_FRAME_TARGET_KEYEXT  0x10u /* TargetGrain carries a KeyExt string (not returned)          */
#define GD_FRAME_INVALIDATION   0x20u /* GD_OPT_WALK_INVALIDATION 1 only: the mask has the
                                         CacheInvalidationHeader bit (any count, zero included).  The
                                         field -- int32 count, then per entry a 24-B SiloAddress and two
                                         UniqueKeys with their KeyExt strings -- was stepped over: every
                                         other output, the mask included, is that of the same frame with
                                         the field cut out (a KeyExt offset stays absolute in buf).  A
                                         negative count or entries that run past the header:
                                         GD_FRAME_MALFORMED alone.  RequestContext, and TargetObserver
                                         ahead of TargetSilo, stay GD_FRAME_FALLBACK.  With the option at
                                         0 (default) the flag is never set and such a frame is
                                         GD_FRAME_FALLBACK.  gd_sniff_frames* reads the entries          */

#define GD_ROUTE_ADDRESSED      5 /* frame address already complete: not looked up (Dispatcher.cs:718) */
#define GD_ROUTE_UNDECODED      6 /* no TargetGrain decoded (absent / fallback / malformed): C# path    */

/* Output arrays, n entries each.  flags and target_grain are required; any other pointer may
 * be NULL (field not extracted).  Absent fields read 0 (direction: 0xFF = null).  Silo
 * addresses are the 24-byte wire form (16-byte IP, int32 port, int32 generation,
 * BinaryTokenStreamWriter.cs:485-513), 4-byte aligned. */
typedef struct gd_frame_fields {
    uint32_t* flags;               /* GD_FRAME_* */
    gd_key*   target_grain;
    uint32_t* mask;                /* HeadersContainer.Headers bits (Message.cs:728-765) */
    gd_key*   target_activation;
    gd_key*   sending_activation;
    gd_key*   sending_grain;
    uint8_t*  target_silo;         /* 24 B per frame */
    uint8_t*  sending_silo;        /* 24 B per frame */
    int64_t*  correlation_id;
    uint8_t*  category;            /* Message.Categories */
    uint8_t*  direction;           /* Message.Directions, 0xFF = null */
} gd_frame_fields;

/* Device pointers; enqueue only.  frame_off[i] = byte offset of frame i in buf. */
int gd_decode_frames_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                            uint32_t n, const gd_frame_fields* d_out);
/* Host pointers (buffer, offsets and outputs); synchronous. */
int gd_decode_frames(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                     const gd_frame_fields* out);
/* Decode -> route -> (optional) bucket, device pointers, enqueue only.  d_out receives the
 * decoded fields (flags + target_grain required).  Statuses are gd_route's plus
 * GD_ROUTE_ADDRESSED / GD_ROUTE_UNDECODED (silo = act = GD_NO_*, trailing bucket).  With an
 * ActivationDirectory (gd_actdir_add), an ADDRESSED frame whose TargetActivation FindTarget finds
 * Valid gets that context as its act and is bucketed with it (IncomingMessageAgent.cs:131-152).
 * d_perm / d_offsets NULL = no bucketing. */
int gd_route_frames_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                           uint32_t n, uint32_t n_act, const gd_frame_fields* d_out, uint32_t* d_silo,
                           uint32_t* d_act, uint8_t* d_status, uint32_t* d_perm, uint32_t* d_offsets);
/* Host-pointer form of gd_route_frames_device (flags + target keys are returned through out
 * when it is non-NULL; perm/offsets NULL = no bucketing); synchronous. */
int gd_route_frames(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                    uint32_t n_act, const gd_frame_fields* out, uint32_t* out_silo, uint32_t* out_act,
                    uint8_t* out_status, uint32_t* out_perm, uint32_t* out_offsets);
/* The same with KeyExt targets (string-keyed grains) routed on the GPU as gd_route_ext does:
 * each TargetGrain's KeyExt string is read from the frame buffer where the decoder found it. */
int gd_route_frames_ext_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                               uint32_t n, uint32_t n_act, const gd_frame_fields* d_out, uint32_t* d_silo,
                               uint32_t* d_act, uint8_t* d_status, uint32_t* d_perm, uint32_t* d_offsets);
int gd_route_frames_ext(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                        uint32_t n_act, const gd_frame_fields* out, uint32_t* out_silo, uint32_t* out_act,
                        uint8_t* out_status, uint32_t* out_perm, uint32_t* out_offsets);

/* ---- membership change ------------------------------------------------
 * GrainDirectoryPartition.Split(predicate, modifyOrigin) (GrainDirectoryPartition.cs:532-570)
 * with the handoff predicate "CalculateTargetSilo(grain) is not me"
 * (GrainDirectoryHandoffManager.cs:212-218), evaluated on the GPU under the installed ring
 * (install the new ring with gd_ring_set first).  "me" = the silos whose partitions this
 * handle holds: keep_silo[s] != 0 (silo indices >= n_keep count as not kept).  Selected live
 * entries are written in slot order; move != 0 also removes them (the RemoveGrain after
 * RegisterMany, :228-232).  KeyExt grains are never selected (their owner needs the C# hash).
 * out_keys == NULL: size query only (*out_n = entries selected, nothing moved).  The merge on
 * the receiving handle is gd_dir_register (GrainDirectoryPartition.Merge, :497-520: entries
 * already present keep their activation and are reported; the host applies the reference's
 * smallest-ActivationId rule to those). */
int gd_dir_split(gd_handle* h, const uint8_t* keep_silo, uint32_t n_keep, int move, gd_key* out_keys,
                 gd_val* out_vals, uint64_t out_capacity, uint64_t* out_n);
/* The same split over the KeyExt table (string-keyed grains): the owner of each entry's stored
 * uniform hash under the installed ring.  Entries in slot order with their KeyExt strings:
 * out_length[i] (GD_KEYEXT_NULL for a null KeyExt), out_offset[i] into out_bytes.  out_keys == NULL:
 * size query (*out_n entries, *out_nbytes string bytes).  Host pointers; the merge on the receiving
 * handle is gd_dir_register_ext. */
int gd_dir_split_ext(gd_handle* h, const uint8_t* keep_silo, uint32_t n_keep, int move, gd_key* out_keys,
                     gd_val* out_vals, uint64_t* out_offset, int32_t* out_length, uint8_t* out_bytes,
                     uint64_t capacity, uint64_t bytes_capacity, uint64_t* out_n, uint64_t* out_nbytes);
/* Same, device output arrays (keep_silo stays a host array); synchronous. */
int gd_dir_split_device(gd_handle* h, const uint8_t* keep_silo, uint32_t n_keep, int move, gd_key* d_out_keys,
                        gd_val* d_out_vals, uint64_t out_capacity, uint64_t* out_n);

/* ---- follower fan-out (BASELINE cfg 4) -----------------------------------
 * ChirperAccount.PublishMessage (Samples/Chirper/ChirperGrains/ChirperAccount.cs:106-147): each
 * publisher sends IChirperSubscriber.NewChirp to every follower, in State.Followers enumeration
 * order (:131-134).  The follower graph is CSR over node ids, where node u is the grain
 * GrainId(type_code, (long)u) (GrainId.cs:72-77): row_off[n_nodes + 1] (u32, row_off[n_nodes] =
 * edges < 2^32), dst[edges] = the followers of u in row_off[u]..row_off[u+1], in enumeration
 * order.  One hop over a frontier of publishers emits, in this order,
 *     for i in 0..n_frontier:  for each follower f of frontier[i]:  (target f, sender frontier[i])
 * Publishers >= n_nodes have no followers.  *out_n = messages emitted (the hop's size; computed
 * on the device and read back, so these calls synchronise).  capacity = room in the outputs;
 * more messages than that is GD_EINVAL with *out_n set (a size query).  All ids are u32. */
/* Expansion only (the multi-GPU path ships (target, sender) to the owner).  d_target == NULL:
 * size query. */
int gd_fanout_expand_device(gd_handle* h, const uint32_t* d_row_off, const uint32_t* d_dst, uint32_t n_nodes,
                            const uint32_t* d_frontier, uint32_t n_frontier, uint32_t* d_target, uint32_t* d_sender,
                            uint64_t capacity, uint64_t* out_n);
/* Fused expansion + route (GrainId formed in registers, K0+K1+K2 as gd_route) + optional
 * bucketing by activation (d_perm / d_offsets NULL = none; as gd_bucket over d_act).
 * d_target may be NULL. */
int gd_fanout_route_bucket_device(gd_handle* h, const uint32_t* d_row_off, const uint32_t* d_dst, uint32_t n_nodes,
                                  const uint32_t* d_frontier, uint32_t n_frontier, int32_t type_code, uint32_t n_act,
                                  uint32_t* d_target, uint32_t* d_sender, uint32_t* d_silo, uint32_t* d_act,
                                  uint8_t* d_status, uint32_t* d_perm, uint32_t* d_offsets, uint64_t capacity,
                                  uint64_t* out_n);
/* Host-pointer form (graph, frontier and outputs in host memory; any output may be NULL
 * except that perm and offsets go together). */
int gd_fanout_route_bucket(gd_handle* h, const uint32_t* row_off, const uint32_t* dst, uint32_t n_nodes,
                           const uint32_t* frontier, uint32_t n_frontier, int32_t type_code, uint32_t n_act,
                           uint32_t* out_target, uint32_t* out_sender, uint32_t* out_silo, uint32_t* out_act,
                           uint8_t* out_status, uint32_t* out_perm, uint32_t* out_offsets, uint64_t capacity,
                           uint64_t* out_n);
/* gd_route_device for GrainId(type_code, (long)node) given node ids (4 B per message instead of
 * a 24-B key): the owner side of the sharded fan-out. */
int gd_route_nodes_device(gd_handle* h, const uint32_t* d_nodes, uint32_t n, int32_t type_code, uint32_t* d_silo,
                          uint32_t* d_act, uint8_t* d_status);
/* gd_pack_by_shard_device for (node, payload) pairs: stable partition by owner silo % n_shards
 * under the installed ring (OutboundMessageQueue.cs:54-131 per target silo). */
int gd_pack_nodes_by_shard_device(gd_handle* h, const uint32_t* d_nodes, const uint32_t* d_payload, uint32_t n,
                                  int32_t type_code, uint32_t n_shards, uint32_t* d_send_nodes,
                                  uint32_t* d_send_payload, uint32_t* d_counts);
/* Next cascade frontier from a hop's bucketing: activations a < n_act with
 * d_offsets[a+1] > d_offsets[a] and d_visited[a] == 0, ascending; marks them visited.
 * d_out holds n_act entries; *out_n = frontier size (synchronises). */
int gd_frontier_next_device(gd_handle* h, const uint32_t* d_offsets, uint32_t n_act, uint8_t* d_visited,
                            uint32_t* d_out, uint32_t* out_n);

/* ---- the sharded fan-out cascade (BASELINE cfg 4 across GPUs: SURVEY 8 f2 over 8 e) ---------
 * Over the library's communicator (gd_comm_init / gd_comm_init_local): rank r owns the directory
 * partitions of silos s % n_ranks == r, as in gd_route_multi; the follower graph is replicated.
 * From `seeds` (the same array on every rank) each rank takes the seeds whose grain it owns, in seed
 * order, and marks them published.  Then per hop, on every rank:
 *   expand its publishers (ChirperAccount.cs:131-134, as gd_fanout_expand_device) -> stable
 *   partition of the (target, sender) pairs by the target's owner rank (the per-silo outbound
 *   queues, OutboundMessageQueue.cs:54-131) -> one grouped send/recv round, 8 B a message ->
 *   route the targets and bucket per activation on the owner, in arrival order = (sender rank,
 *   sender emission order) -> the next publishers: this rank's activations that received a chirp
 *   and have not published yet, ascending (gd_frontier_next_device).
 * Collective: every rank calls it with the same seeds, hops and n_act.  out[hops] (may be NULL):
 * device pointers into library-owned buffers, valid until the next call on the handle,
 * gd_comm_destroy or gd_destroy.  Blocks the host twice per hop (the hop's size, the counts round). */
typedef struct gd_fanout_hop {
    uint32_t        n_frontier;   /* this rank's publishers of the hop                        */
    const uint32_t* frontier;
    uint64_t        n_sent;       /* messages they emitted                                    */
    uint32_t        n_recv;       /* messages delivered here (this rank owns their grain)     */
    const uint32_t* target;       /* [n_recv] follower node, arrival order                    */
    const uint32_t* sender;       /* [n_recv] publisher node                                  */
    const uint32_t* src;          /* [n_recv] sending rank                                    */
    const uint32_t* silo;         /* [n_recv] route results (as gd_route_nodes_device)        */
    const uint32_t* act;
    const uint8_t*  status;
    const uint32_t* perm;         /* [n_recv] stable per-activation order                     */
    const uint32_t* offsets;      /* [n_act + 2]                                              */
} gd_fanout_hop;
int gd_fanout_multi_device(gd_handle* h, const uint32_t* d_row_off, const uint32_t* d_dst, uint32_t n_nodes,
                           const uint32_t* d_seeds, uint32_t n_seeds, int32_t type_code, uint32_t n_act,
                           uint32_t hops, gd_fanout_hop* out);
/* The same cascade over a partitioned follower graph: each rank holds only the
 * follower lists of the grains it owns -- the publishers a rank expands are always its own activations
 * (a chirp is enqueued on its follower's activation, on the follower's directory owner, which then
 * publishes; ChirperAccount.cs:131-134) -- so per-rank graph memory is ~1/n_ranks.  Row i of this
 * rank's CSR (d_row_off[n_rows + 1], d_dst = follower node ids) is local activation i, whose node is
 * d_node_of[i]; the directory must map each owned node to its row (act = i), with rows in ascending
 * node order so that publishers run in the replicated form's order (the hops are then bit-identical
 * to gd_fanout_multi_device's).  Every seed needs a live activation on its owner (else GD_EINVAL).
 * n_act = n_rows: buckets and offsets are over local rows; frontier, target and sender are node ids. */
int gd_fanout_multi_part_device(gd_handle* h, const uint32_t* d_row_off, const uint32_t* d_dst, uint32_t n_rows,
                                const uint32_t* d_node_of, const uint32_t* d_seeds, uint32_t n_seeds,
                                int32_t type_code, uint32_t hops, gd_fanout_hop* out);
/* Host graph and seeds (uploaded per call); returns with the cascade done. */
int gd_fanout_multi(gd_handle* h, const uint32_t* row_off, const uint32_t* dst, uint32_t n_nodes,
                    const uint32_t* seeds, uint32_t n_seeds, int32_t type_code, uint32_t n_act, uint32_t hops,
                    gd_fanout_hop* out);
/* The single-GPU cascade inside the library (BASELINE cfg 4 on one GPU; what gd_fanout_route_bucket
 * + gd_frontier_next do hop by hop from the host): `seeds` publish in seed order, then per hop the
 * fused expand + route (ChirperAccount.cs:131-134), the bucketing per activation and the next
 * publishers (this handle's activations that received a chirp and have not published, ascending).
 * Node u = activation u (n_act >= the nodes that have activations).  One host read-back a hop (the
 * next hop's message and publisher counts together, the frontier's size staying on the device until
 * then).  out[hops] (may be NULL): device pointers into library buffers as gd_fanout_multi_device's
 * (src = NULL); gd_fanout_multi_fetch copies a hop out (src as zeros). */
int gd_fanout_cascade_device(gd_handle* h, const uint32_t* d_row_off, const uint32_t* d_dst, uint32_t n_nodes,
                             const uint32_t* d_seeds, uint32_t n_seeds, int32_t type_code, uint32_t n_act,
                             uint32_t hops, gd_fanout_hop* out);
/* Copy hop `hop` of the last cascade to host arrays sized from its gd_fanout_hop (any may be NULL). */
int gd_fanout_multi_fetch(gd_handle* h, uint32_t hop, uint32_t* frontier, uint32_t* target, uint32_t* sender,
                          uint32_t* src, uint32_t* silo, uint32_t* act, uint8_t* status, uint32_t* perm,
                          uint32_t* offsets);

/* ---- non-owner directory cache -------------------------------------------
 * AdaptiveGrainDirectoryCache over LRU<GrainId, entry> (src/Orleans.Runtime/GrainDirectory/
 * AdaptiveGrainDirectoryCache.cs:7-140, src/Orleans.Core/Utils/LRU.cs) on the LocalLookup path
 * (LocalGrainDirectory.cs:797-850).  Configured (max_size > 0), gd_route / gd_route_device /
 * gd_route_bucket[_device] run LocalLookup per message: a grain whose ring owner is a local
 * silo (local_silo[owner] != 0) is probed in this handle's directory partition; any other grain
 * in the cache.  A cache hit whose silo is not valid (valid_silo[silo] == 0, IsValidSilo) is
 * GD_ROUTE_MISS, as is a cache miss (silo = ring owner, act = GD_NO_ACTIVATION).  The LRU is the
 * reference's exactly: every hit and every add takes the next generation (hits in batch order),
 * AdjustSize evicts the lowest generation while count >= max_size.  max_size 0 = no cache
 * (whole-node mode: every grain is probed in this handle's table).  The frame and micro-batch
 * paths run LocalLookup too (the micro-batch eagerly in this mode); the fan-out paths do not
 * consult the cache. */
typedef struct gd_cache_stats {
    uint64_t count;             /* live entries (LRU.Count)                       */
    uint64_t accesses;          /* NumAccesses                                     */
    uint64_t hits;              /* NumHits                                         */
    uint64_t next_generation;   /* LRU.nextGeneration                              */
    uint64_t max_size;
    uint64_t capacity;          /* table slots                                     */
} gd_cache_stats;
int gd_cache_configure(gd_handle* h, uint32_t max_size, const uint8_t* local_silo, const uint8_t* valid_silo,
                       uint32_t n_silos);
/* Membership change: new local / valid silo masks; entries stay (the maintainer refreshes them). */
int gd_cache_set_silos(gd_handle* h, const uint8_t* local_silo, const uint8_t* valid_silo, uint32_t n_silos);
/* AddOrUpdate(key, value, version) for each entry in order (after a remote lookup, :920). */
int gd_cache_add(gd_handle* h, const gd_key* keys, const gd_val* vals, const int32_t* versions, uint32_t n);
/* Remove (:79-83); out_removed may be NULL. */
int gd_cache_remove(gd_handle* h, const gd_key* keys, uint32_t n, uint8_t* out_removed);
/* LookUp (:90-109) in order: value + version (ETag) of hits. */
int gd_cache_lookup(gd_handle* h, const gd_key* keys, uint32_t n, gd_val* out_vals, int32_t* out_versions,
                    uint8_t* out_found);
int gd_cache_clear(gd_handle* h);
int gd_cache_stats_get(gd_handle* h, gd_cache_stats* out);
/* KeyValues (:111-127) with each entry's generation, in slot order; keys NULL = size query. */
int gd_cache_entries(gd_handle* h, gd_key* keys, gd_val* vals, int32_t* versions, uint64_t* generations,
                     uint64_t capacity, uint64_t* out_n);
/* KeyExt grains (string, compound keys, geo clients: UniqueKey.HasKeyExt) in the cache, keyed by their
 * KeyExt as UniqueKey.Equals is (UniqueKey.cs:245-251) and homed by the KeyExt uniform hash
 * (UniqueKey.cs:272-336).  gd_route_ext / gd_route_bucket_ext[_device] / gd_route_frames_ext* in
 * LocalLookup mode route KeyExt grains the same way as the three-word ones: the owner by the KeyExt
 * hash, a local owner's grains in this handle's KeyExt partition (gd_dir_register_ext), the others
 * in the cache (AdaptiveGrainDirectoryCache.cs:93-110), every hit of the batch numbered in batch
 * order.  One LRU holds both kinds (one generation sequence, one max_size).  `ext` is read for
 * KeyExt-category keys only; GD_KEYEXT_NULL there is the three-word entry, GD_KEYEXT_HOST is
 * GD_EINVAL.  The plain forms above treat a KeyExt-category key as KeyExt null. */
int gd_cache_add_ext(gd_handle* h, const gd_key* keys, const gd_key_ext* ext, const gd_val* vals,
                     const int32_t* versions, uint32_t n);
int gd_cache_remove_ext(gd_handle* h, const gd_key* keys, const gd_key_ext* ext, uint32_t n, uint8_t* out_removed);
int gd_cache_lookup_ext(gd_handle* h, const gd_key* keys, const gd_key_ext* ext, uint32_t n, gd_val* out_vals,
                        int32_t* out_versions, uint8_t* out_found);
/* gd_cache_entries with each entry's KeyExt: ext_len[k] (GD_KEYEXT_NULL for a three-word key), its
 * UTF-8 bytes at ext_bytes + ext_off[k]; *out_bytes = the bytes all strings need.  keys NULL = size
 * query (*out_n, *out_bytes). */
int gd_cache_entries_ext(gd_handle* h, gd_key* keys, gd_val* vals, int32_t* versions, uint64_t* generations,
                         int32_t* ext_len, uint64_t* ext_off, uint8_t* ext_bytes, uint64_t capacity,
                         uint64_t bytes_capacity, uint64_t* out_n, uint64_t* out_bytes);

/* ---- the directory cache's maintainer -----------------------------------------
 * What makes the cache adaptive: per entry NumAccesses, LastRefreshed and ExpirationTimer
 * (AdaptiveGrainDirectoryCache.cs:15-35), and AdaptiveDirectoryCacheMaintainer.Run
 * (AdaptiveDirectoryCacheMaintainer.cs:42-131) over them -- the expiry scan, the per-owner request
 * lists (SendBatchCacheRefreshRequests :133-153, BuildGrainAndETagList :202-224), the owner's
 * LookUpMany (RemoteGrainDirectory.cs:65-96) and the response pass (ProcessCacheRefreshResponse
 * :155-193).  Created (:13) is written by the reference and never read on this path: it is not
 * stored.  Times are DateTime.Ticks passed in; one `now` stands for every DateTime.UtcNow a call
 * would read.
 *
 * The cache clock (gd_cache_clock_set; scan and apply set it to their `now` first) is the UtcNow of
 * the add path: every entry gd_cache_add* creates -- a replaced key's too, AddOrUpdate builds a new
 * entry (:74-80) -- gets LastRefreshed = clock, ExpirationTimer = initial, NumAccesses = 0.  Every
 * LookUp hit (gd_cache_lookup* and every LocalLookup route form) is one NumAccesses++ on its entry
 * (:106), duplicates in a batch counted each.
 *
 * gd_cache_maintain_configure stores the constructor's parameters (:63-70); before it they are 30 s,
 * 240 s and 2.0 (GrainDirectoryOptions.cs:31-55).  GD_EINVAL: no cache configured, a negative tick
 * count, growth not finite or <= 0, (double)max(initial, max) * growth >= 2^62 (the checked overflow
 * of StandardExtensions.Multiply, refused up front). */
int gd_cache_maintain_configure(gd_handle* h, int64_t initial_ticks, int64_t max_ticks, double growth, int64_t now);
int gd_cache_clock_set(gd_handle* h, int64_t now);
/* LastRefreshed, ExpirationTimer and NumAccesses of every entry in the slot order of gd_cache_entries
 * (the two dumps zip together); refreshed NULL = size query. */
int gd_cache_entries_age(gd_handle* h, int64_t* refreshed, int64_t* timer, int32_t* num_accesses, uint64_t capacity,
                         uint64_t* out_n);

/* Run's loop at `now`.  The reference enumerates a ConcurrentDictionary, whose order is unspecified;
 * here the enumeration order is ascending cache slot, the order of gd_cache_entries.  Per live entry,
 * owner = CalculateTargetSilo under the installed ring (a KeyExt entry by its KeyExt hash):
 *   GD_CM_SELF_OWNED  local_silo[owner] != 0: removed (:79-86)
 *   GD_CM_FRESH       now < LastRefreshed + ExpirationTimer: nothing (:95-99; IsExpired is >=)
 *   GD_CM_DROPPED     expired and NumAccesses == 0: removed (:100-105)
 *   GD_CM_REFRESH     expired and accessed: NumAccesses = 0, appended to its owner's list (:106-117)
 * The lists: owners in order of first appearance in the enumeration, one owner's candidates in
 * enumeration order; candidate j of that grouped order takes generation next_generation + j + 1
 * (BuildGrainAndETagList's cache.Get is LRU.TryGetValue, LRU.cs:124-163; NumAccesses and the
 * statistics are not touched).  out_counts[5]: entries seen, then the four classes (cnt1..cnt4 of :63
 * are [1], [2], [3], [4]).
 *
 * The scan changes the cache, so it runs once and holds its lists in library buffers until the next
 * scan on the handle: gd_cache_scan reports their sizes (the size query), gd_cache_scan_fetch copies
 * them out -- owner[n_owners], offsets[n_owners + 1], and per candidate keys, etags, slots, ext_len
 * (GD_KEYEXT_NULL for a three-word key) and ext_off into ext_bytes, as gd_cache_entries_ext.  Any
 * output of the fetch may be NULL.  gd_cache_scan_device gives the same lists as device pointers. */
#define GD_CM_SEEN       0
#define GD_CM_SELF_OWNED 1
#define GD_CM_FRESH      2
#define GD_CM_DROPPED    3
#define GD_CM_REFRESH    4
typedef struct gd_cache_scan_result {
    uint64_t counts[5];
    uint32_t n_owners, n;          /* request lists, candidates                                    */
    uint64_t ext_bytes_len;
    const uint32_t* owner;         /* device: [n_owners] silo index                                */
    const uint32_t* offsets;       /* device: [n_owners + 1]                                       */
    const gd_key* keys;            /* device: [n]                                                  */
    const int32_t* etags;          /* device: [n]                                                  */
    const uint32_t* slots;         /* device: [n] cache slot                                       */
    const int32_t* ext_len;        /* device: [n]                                                  */
    const uint32_t* ext_off;       /* device: [n] byte offset in ext_bytes                         */
    const uint8_t* ext_bytes;      /* device: [ext_bytes_len]                                      */
} gd_cache_scan_result;
int gd_cache_scan_device(gd_handle* h, int64_t now, gd_cache_scan_result* out);
int gd_cache_scan(gd_handle* h, int64_t now, uint64_t* out_counts, uint32_t* out_n_owners, uint32_t* out_n,
                  uint64_t* out_bytes);
int gd_cache_scan_fetch(gd_handle* h, uint32_t* owner, uint32_t* offsets, gd_key* keys, int32_t* etags,
                        uint32_t* slots, int32_t* ext_len, uint64_t* ext_off, uint8_t* ext_bytes,
                        uint32_t owner_capacity, uint32_t capacity, uint64_t bytes_capacity);

/* The owner side, LookUpMany per item (items are independent).  cur = GetGrainETag
 * (GrainDirectoryPartition.cs:479-491): the entry's VersionTag, -1 without one.
 *   GD_LM_SAME     cur == etag and cur != -1: out_tags = cur, no value
 *   GD_LM_ABSENT   cur == -1: out_tags = -1
 *   GD_LM_UPDATED  otherwise: out_tags = the VersionTag, out_vals as gd_dir_lookup_tagged gives it,
 *                  {GD_NO_ACTIVATION, GD_NO_SILO} for an entry whose silo fails IsValidSilo (the filtered
 *                  list is empty, not null, and the requester caches the empty list:
 *                  RemoteGrainDirectory.cs:83-88, GrainDirectoryPartition.cs:427-434)
 *   GD_LM_HOST     a changed GD_ACT_MULTI entry (its instance list lives in C#) or any KeyExt-category key
 *                  (the KeyExt partition carries no VersionTags): answered in C#
 * The equality test comes first, so an unchanged multi-activation entry is GD_LM_SAME. */
#define GD_LM_SAME    0
#define GD_LM_ABSENT  1
#define GD_LM_UPDATED 2
#define GD_LM_HOST    3
int gd_dir_lookup_many_device(gd_handle* h, const gd_key* d_keys, const int32_t* d_etags, uint32_t n,
                              uint8_t* d_kind, gd_val* d_vals, int32_t* d_tags);
int gd_dir_lookup_many(gd_handle* h, const gd_key* keys, const int32_t* etags, uint32_t n, uint8_t* out_kind,
                       gd_val* out_vals, int32_t* out_tags);

/* The response, ProcessCacheRefreshResponse per item in batch order at `now`:
 *   GD_LM_UPDATED  AddOrUpdate(key, value, tag): LRU.Add -- AdjustSize, then a new entry with a new
 *                  generation, LastRefreshed = now, ExpirationTimer = initial, NumAccesses = 0; a value of
 *                  silo GD_NO_SILO is the empty address list (dumps show it as {GD_NO_ACTIVATION, 0xFFFF};
 *                  routes miss on it)
 *   GD_LM_ABSENT   Remove
 *   GD_LM_SAME     MarkAsFresh (AdaptiveGrainDirectoryCache.cs:127-136): if still cached, the next
 *                  generation, ExpirationTimer = min(max, (long)((double)timer * growth)), LastRefreshed = now
 *   GD_LM_HOST     skipped
 * out_status (may be NULL) says what happened.  Keys of one batch are distinct: two items that find one
 * cached entry are GD_EINVAL and change nothing.  ext (may be NULL) keys KeyExt entries as gd_cache_add_ext.
 * A batch without UPDATED items runs on the device with no host round trip before its results; one with
 * them goes through the add path's host simulation and is exact under eviction (an UPDATED item's
 * AdjustSize may evict a key whose SAME comes later: GD_CR_NOT_PRESENT).  The device form applies the SAME /
 * ABSENT / HOST items only and marks UPDATED ones GD_CR_DEFERRED for the host form; a duplicate there
 * changes nothing and is reported by the call's return after it synchronises. */
#define GD_CR_UPDATED     0
#define GD_CR_REMOVED     1
#define GD_CR_NOT_PRESENT 2
#define GD_CR_FRESHENED   3
#define GD_CR_SKIPPED     4
#define GD_CR_DEFERRED    5
int gd_cache_refresh_apply_device(gd_handle* h, int64_t now, const gd_key* d_keys, const gd_key_ext* d_ext,
                                  const uint8_t* d_kind, uint32_t n, uint8_t* d_status);
int gd_cache_refresh_apply(gd_handle* h, int64_t now, const gd_key* keys, const gd_key_ext* ext, const uint8_t* kind,
                           const gd_val* vals, const int32_t* tags, uint32_t n, uint8_t* out_status);

/* ---- membership change: IsValidSilo, VersionTag, silo removal, handoff merge ----
 * GrainDirectoryPartition.IsValidSilo (GrainDirectoryPartition.cs:242-245, the membership oracle's
 * IsFunctionalDirectory): valid[s] != 0 for every silo index s < n_silos that is a functional
 * directory member; silo indices >= n_silos count as valid; n_silos = 0 = every silo valid (the
 * default).  With the mask set:
 *   - gd_dir_register / gd_dir_register_device / gd_dir_register_ext (AddSingleActivation, :304-326)
 *     and gd_dir_upsert (AddActivation, :274-302) skip an item whose silo is not valid (no entry, out
 *     value {GD_NO_ACTIVATION, GD_NO_SILO}, not inserted);
 *   - LookUpActivations (:385-441) filters an entry on an invalid silo: routes give GD_ROUTE_MISS (an
 *     empty address list fails FastLookup, Catalog.cs:1321-1330), gd_dir_lookup_tagged reports it. */
int gd_dir_set_valid_silos(gd_handle* h, const uint8_t* valid, uint32_t n_silos);
/* LookUpActivations with its VersionTag: out_found[i] = 0 no entry (tag 0, the AddressesAndTag
 * default), 1 an entry with a valid address (out_vals), 2 an entry whose activation's silo is not
 * valid (empty address list; tag still given).  VersionTags are non-negative int32.  The reference
 * draws a fresh rand.Next() whenever a grain's entry changes (GrainInfo :106,120,135,154); this
 * library gives a deterministic 31-bit function of (the mutating call's sequence number, the grain's
 * uniform hash), changed exactly where the reference draws one.  Host pointers. */
int gd_dir_lookup_tagged(gd_handle* h, const gd_key* keys, uint32_t n, gd_val* out_vals, int32_t* out_tags,
                         uint8_t* out_found);
/* RemoveServer's AdjustLocalDirectory (LocalGrainDirectory.cs:340-361): every entry whose activation
 * lives on one of the removed silos is dropped (RemoveActivation, Force; single-activation grains lose
 * their grain).  Multi-activation entries (GD_ACT_MULTI) are counted in *out_multi and left to the host
 * (their instance silos live in C#).  In LocalLookup mode (gd_cache_configure) also AdjustLocalCache
 * (:371-385) under the installed ring -- install the ring without the removed silos first: cache
 * entries pointing at a removed silo or whose grain a local silo now owns are removed
 * (*out_cache_removed).  KeyExt entries follow the same rule.  Any out pointer may be NULL. */
int gd_dir_remove_silos(gd_handle* h, const uint32_t* silos, uint32_t n_silos, uint64_t* out_removed,
                        uint64_t* out_multi, uint64_t* out_cache_removed);
/* The ActivationId (ActivationId.cs; a UniqueKey, NewId = Guid with Category None) of host activation
 * indices: ids[i] for acts[i].  gd_dir_merge orders activations by it (UniqueKey.CompareTo,
 * UniqueKey.cs:255-265: TypeCodeData, N0, N1).  Host pointers. */
int gd_activation_ids_set(gd_handle* h, const uint32_t* acts, const gd_key* ids, uint32_t n);
/* GrainDirectoryPartition.Merge (GrainDirectoryPartition.cs:497-522) of a received partition (the copy
 * merged by GrainDirectoryHandoffManager.ProcessSiloRemoveEvent, :125-158): one item per grain (a
 * duplicated grain fails with GD_EINVAL and changes nothing).  Per item:
 *   GD_MERGE_INSERTED  the grain was absent: the incoming entry is added with its VersionTag
 *                      (tags[i]; tags NULL = a new tag)
 *   GD_MERGE_SAME      the same activation is registered: nothing changes (GrainInfo.Merge :146)
 *   GD_MERGE_KEPT      single-activation grain, the incoming ActivationId is the lower: it replaces the
 *                      existing entry (GrainInfo.Merge :159-176); out_dropped[i] = the displaced one
 *   GD_MERGE_DROPPED   the existing ActivationId is the lower: out_dropped[i] = the incoming activation
 *   GD_MERGE_UNION     a multi-instance grain holding one instance here meets another: both kept (below)
 *   GD_MERGE_HOST      a grain with several instances on either side (its lists are unioned by C#)
 * out_dropped lists what Catalog.DeleteActivations gets per silo (:514-518); {GD_NO_*} otherwise.  Both
 * activations of a conflict need an ActivationId (gd_activation_ids_set), else GD_EINVAL.  No
 * IsValidSilo check (Merge has none).  Host pointers; out_dropped may be NULL. */
#define GD_MERGE_INSERTED 0
#define GD_MERGE_KEPT     1
#define GD_MERGE_SAME     2
#define GD_MERGE_DROPPED  3
#define GD_MERGE_HOST     4
/* GD_MERGE_UNION     the grain here is a multi-instance one (AddActivation, SingleInstance false) holding
 *                    one instance, and the incoming instance is another: GrainInfo.Merge unions the lists
 *                    (:141-152) and keeps both; the entry becomes GD_ACT_MULTI with a new VersionTag and
 *                    the host adds the incoming instance to its list */
#define GD_MERGE_UNION    5
/* tags[i] | GD_MERGE_TAG_MULTI_INSTANCE: the incoming GrainInfo is not SingleInstance (an AddActivation
 * grain holding one instance); partitionData.Add keeps it so (tags NULL: single unless GD_ACT_MULTI). */
#define GD_MERGE_TAG_MULTI_INSTANCE 0x80000000u
int gd_dir_merge(gd_handle* h, const gd_key* keys, const gd_val* vals, const int32_t* tags, uint32_t n,
                 uint8_t* out_status, gd_val* out_dropped);

/* ---- multi-rank directory handoff (SURVEY 8 f4 over 8 e) ------------------------------------------
 * After a membership change (the new ring installed on every rank with gd_ring_set), each rank splits
 * off the entries whose new owner silo it does not host (keep_silo as gd_dir_split, removed here), they
 * travel to the owner's rank (silo % n_ranks) in one grouped round over the library's communicator with
 * their ActivationId (gd_activation_ids_set) and VersionTag, and the receiver applies them as the
 * reference distinguishes the two events (GrainDirectoryHandoffManager.cs):
 *   GD_HANDOFF_ADD     ProcessSiloAddEvent (:195-245): RegisterMany(singleActivation: true) --
 *                      AddSingleActivation, the first registration wins (GrainDirectoryPartition.cs:304-326)
 *   GD_HANDOFF_REMOVE  ProcessSiloRemoveEvent (:125-158): GrainDirectoryPartition.Merge (:497-522) --
 *                      GrainInfo.Merge keeps the lowest ActivationId (:139-179), the incoming VersionTag
 *                      and SingleInstance flag travel with the entry
 * Received entries take this handle's activation indices act_base + j (j = arrival position; their
 * ActivationIds are set at those indices as by gd_activation_ids_set); multi-activation entries stay
 * GD_ACT_MULTI (their instance lists are the host's).  Per received entry, status:
 *   GD_MERGE_INSERTED  the grain was absent here: the entry is added
 *   GD_MERGE_SAME      the same ActivationId already holds the grain
 *   GD_MERGE_KEPT      (REMOVE) the incoming ActivationId is the lower: it replaces the holder;
 *                      dropped = the displaced {act, silo} (Catalog.DeleteActivations on that silo)
 *   GD_MERGE_DROPPED   REMOVE: the holder's ActivationId is the lower, dropped = the incoming entry;
 *                      ADD: another activation holds the grain (first registration wins) or the silo is
 *                      not valid, dropped = the holder (none when refused)
 *   GD_MERGE_HOST      a multi-activation entry on either side: C# unions the instance lists
 * Collective over the communicator; synchronous.  The result's device arrays (arrival order = sender
 * rank, sender slot order) stay valid until the next call, gd_comm_destroy or gd_destroy. */
#define GD_HANDOFF_ADD    0
#define GD_HANDOFF_REMOVE 1
typedef struct gd_handoff_result {
    uint64_t        n_sent;       /* entries this rank split off and sent              */
    uint32_t        n_recv;       /* entries received                                  */
    const gd_key*   recv_keys;    /* [n_recv] GrainIds                                 */
    const gd_key*   recv_ids;     /* [n_recv] ActivationIds (zero for multi-activation) */
    const uint32_t* recv_act;     /* [n_recv] activation index here (GD_ACT_MULTI kept) */
    const uint32_t* recv_silo;    /* [n_recv] silo index (bit 31: a multi-activation entry) */
    const uint32_t* recv_src;     /* [n_recv] sending rank                             */
    const uint8_t*  status;       /* [n_recv] GD_MERGE_*                               */
    const gd_val*   dropped;      /* [n_recv] see above; {GD_NO_*} otherwise           */
} gd_handoff_result;
int gd_dir_handoff_multi(gd_handle* h, const uint8_t* keep_silo, uint32_t n_keep, int event, uint32_t act_base,
                         gd_handoff_result* out);
/* Host copies of the last handoff's received entries (any pointer may be NULL; silos without the
 * multi-activation mark). */
int gd_dir_handoff_fetch(gd_handle* h, gd_key* keys, gd_key* ids, uint32_t* acts, uint32_t* silos, uint32_t* src,
                         uint8_t* status, gd_val* dropped);

/* ---- receive path: ActivationDirectory + IncomingMessageAgent -----------------
 * ActivationDirectory (src/Orleans.Runtime/Catalog/ActivationDirectory.cs): ActivationId -> the
 * host's scheduling-context index + flags, in an HBM table.  Activations (RecordNewTarget :86-93) and
 * system targets (RecordNewSystemTarget :95-98, flag GD_ACTDIR_SYSTEM_TARGET) share one table and
 * one context index space; FindTarget (:41-45) sees only activations, FindSystemTarget (:47-51) only
 * system targets.  Use the grain directory's activation index as the context index of a local
 * activation, so gd_route_frames' addressed frames and gd_bucket agree. */
#define GD_ACTDIR_VALID            1u  /* ActivationData.State == Valid                          */
#define GD_ACTDIR_SYSTEM_TARGET    2u  /* an entry of systemTargets                               */
#define GD_ACTDIR_STATELESS_WORKER 4u  /* IsStatelessWorker: the *_StatelessWorker limits apply    */
/* TryAdd (first add of an ActivationId wins); out_added may be NULL. */
int gd_actdir_add(gd_handle* h, const gd_key* act_ids, const uint32_t* ctx, const uint8_t* flags, uint32_t n,
                  uint8_t* out_added);
/* TryRemove (RemoveTarget :116-131); out_removed may be NULL. */
int gd_actdir_remove(gd_handle* h, const gd_key* act_ids, uint32_t n, uint8_t* out_removed);
/* State changes (ActivationData.SetState): new flags, batch order (last wins); out_found may be NULL. */
int gd_actdir_set_flags(gd_handle* h, const gd_key* act_ids, const uint8_t* flags, uint32_t n, uint8_t* out_found);
int gd_actdir_lookup(gd_handle* h, const gd_key* act_ids, uint32_t n, uint32_t* out_ctx, uint8_t* out_flags,
                     uint8_t* out_found);
int gd_actdir_clear(gd_handle* h);
int gd_actdir_count(gd_handle* h, uint64_t* out_live);

/* IncomingMessageAgent.ReceiveMessage (IncomingMessageAgent.cs:92-170) for a batch in arrival order.
 * Per message, from TargetGrain (its category), TargetActivation and Direction (NULL array = every
 * message a Request; 0xFF = header absent = Request, Message.cs:113-116):
 *   GD_RECV_ACTIVATION      FindTarget found a Valid activation: enqueued on its context
 *   GD_RECV_SYSTEM_TARGET   FindSystemTarget found it, Request or Response: enqueued on its context
 *   GD_RECV_NULL_CONTEXT    no activation, or not Valid: EnqueueReceiveMessage(msg, null, null)
 *   GD_RECV_REJECT_UNKNOWN  system target not active here: rejection response (Unrecoverable)
 *   GD_RECV_REJECT_OVERLOADED  CheckOverloaded's hard limit (ActivationData.cs:616-649), see limits
 *   GD_RECV_DROPPED         system target message neither Request nor Response (logged, dropped)
 *   GD_RECV_UNDECODED       (frames) no complete decoded address: C# deserializes it
 * out_ctx[i] = the bucket it is enqueued in: the context index (< n_ctx), n_ctx for the null context,
 * GD_NO_ACTIVATION when not enqueued.  perm / offsets (both or neither): the stable bucketing of the
 * batch over n_ctx + 2 buckets -- contexts, the null context, then the messages not enqueued -- each
 * in arrival order (WorkItemGroup FIFO, WorkItemGroup.cs:174-201); offsets has n_ctx + 3 entries.
 * limits (NULL = none, the default options): request_count[c] = GetRequestCount() of context c when
 * the batch starts (n_ctx entries), hard limits as SiloMessagingOptions' MaxEnqueuedRequestsHardLimit
 * (_StatelessWorker); <= 0 = no limit.  Every enqueued message of an activation counts
 * (IncrementEnqueuedOnDispatcherCount), as when the agent thread enqueues the batch before a worker
 * runs any of it.  The limits apply whether or not perm / offsets are asked for.
 * Every context index gd_actdir_add stored for an entry the batch finds must be < n_ctx: a larger one
 * fails the call with GD_EINVAL (the *_device forms: the next gd_synchronize), the message left
 * un-enqueued with GD_RECV_UNDECODED. */
#define GD_RECV_ACTIVATION        0
#define GD_RECV_SYSTEM_TARGET     1
#define GD_RECV_NULL_CONTEXT      2
#define GD_RECV_REJECT_UNKNOWN    3
#define GD_RECV_REJECT_OVERLOADED 4
#define GD_RECV_DROPPED           5
#define GD_RECV_UNDECODED         6
typedef struct gd_recv_limits {
    const uint32_t* request_count;   /* [n_ctx]; device memory for the *_device entry points */
    int32_t hard_limit;
    int32_t hard_limit_stateless_worker;
} gd_recv_limits;
int gd_receive(gd_handle* h, const gd_key* target_grain, const gd_key* target_activation, const uint8_t* direction,
               uint32_t n, uint32_t n_ctx, const gd_recv_limits* limits, uint32_t* out_ctx, uint8_t* out_status,
               uint32_t* out_perm, uint32_t* out_offsets);
int gd_receive_device(gd_handle* h, const gd_key* d_target_grain, const gd_key* d_target_activation,
                      const uint8_t* d_direction, uint32_t n, uint32_t n_ctx, const gd_recv_limits* limits,
                      uint32_t* d_ctx, uint8_t* d_status, uint32_t* d_perm, uint32_t* d_offsets);
/* The same straight from the receive buffer (frames as gd_route_frames): decode -> ReceiveMessage ->
 * bucketing.  d_out may be NULL or name the decoded fields wanted. */
int gd_receive_frames_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                             uint32_t n, uint32_t n_ctx, const gd_recv_limits* limits, const gd_frame_fields* d_out,
                             uint32_t* d_ctx, uint8_t* d_status, uint32_t* d_perm, uint32_t* d_offsets);
int gd_receive_frames(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                      uint32_t n_ctx, const gd_recv_limits* limits, const gd_frame_fields* out, uint32_t* out_ctx,
                      uint8_t* out_status, uint32_t* out_perm, uint32_t* out_offsets);

/* ---- sender queues ------------------------------------------------
 * OutboundMessageQueue.SendMessage (OutboundMessageQueue.cs:54-131) for a batch that Dispatcher.
 * AddressMessage (gd_route) has addressed: which sender queue every message goes on, and the batch as
 * one contiguous, ordered index list per queue.  Per message, in the reference's order:
 *   GD_SEND_HELD          route status given and none of GD_ROUTE_OK / _SYSTEM_TARGET / _MEMBERSHIP: the
 *                         message has no address yet (slow path, KeyExt, multi-activation, undecoded)
 *   GD_SEND_EXPIRED       ttl != GD_TTL_NONE and ttl <= 0 (Message.IsExpired, Message.cs:293-302; ttl =
 *                         TimeToLive in TimeSpan ticks when the batch is sent): dropped
 *   GD_SEND_NO_SILO       silo == GD_NO_SILO (:82-87): rejection, Unrecoverable
 *   GD_SEND_UNKNOWN_SILO  silo >= n_silos: not in the configured silo table
 *   GD_SEND_LOOPBACK      silo == gd_config.my_silo (:90-95): bucket 0, InboundQueue.PostMessage
 *   GD_SEND_QUEUED        category 0 (Ping, Message.cs:75-80): bucket 1, the ping sender; category 1
 *                         (System): bucket 2, the system sender; any other byte (the C# default: branch,
 *                         Application = 2): bucket 3 + Math.Abs(silo_hash[silo]) % n_queues (:125)
 *   GD_SEND_THROWS        ... unless silo_hash[silo] == INT32_MIN, whose Math.Abs throws
 *                         OverflowException (checked before the modulo, as in .NET)
 * Everything but LOOPBACK and QUEUED lands in the trailing bucket 3 + n_queues, told apart by status.
 * category NULL = every message Application; ttl NULL = no message has a TTL; route status NULL =
 * nothing is held.  out_queue[i] = the bucket id; perm[n] = the message indices grouped by bucket, each
 * bucket in batch order (every sender is a FIFO, SiloMessageSender.QueueRequest); offsets[n_queues + 5]
 * = the bucket starts, offsets[n_queues + 4] = n.  out_queue, and perm + offsets together, may be NULL
 * (perm + offsets NULL: classification only); one of perm / offsets without the other is GD_EINVAL.
 * n == 0 is valid and fills offsets with zeros.  n <= 2^31.
 * gd_send_configure: silo_hash[s] = gd_silo_consistent_hash of silo index s (host pointer), 1 <= n_silos
 * <= 65,536, 1 <= n_queues <= 1,024 (SiloMessagingOptions.SiloSenderQueues), else GD_EINVAL; may be
 * called again (the silo table grows); synchronizes the handle.  The batch calls return GD_ESTATE before
 * it (a NULL handle has no configuration: GD_ESTATE too, after the argument checks).
 * Left to C#: the stopped flag (:58-62), QueuedTime, the ShouldDrop test hook, and MessageCenter.SendMessage's
 * IsBlockingApplicationMessages filter (MessageCenter.cs:177-191).  The gateway proxy check (:77) is
 * gd_gateway_send_queues (the gateway block below); these calls run the rule without it. */
#define GD_TTL_NONE INT64_MAX           /* TimeToLive has no value */
#define GD_SEND_QUEUED       0
#define GD_SEND_LOOPBACK     1
#define GD_SEND_EXPIRED      2
#define GD_SEND_NO_SILO      3
#define GD_SEND_UNKNOWN_SILO 4
#define GD_SEND_THROWS       5
#define GD_SEND_HELD         6
int gd_send_configure(gd_handle* h, const int32_t* silo_hash, uint32_t n_silos, uint32_t n_queues);
int gd_send_queues_device(gd_handle* h, const uint32_t* d_silo, const uint8_t* d_route_status,
                          const uint8_t* d_category, const int64_t* d_ttl, uint32_t n, uint8_t* d_send_status,
                          uint32_t* d_queue, uint32_t* d_perm, uint32_t* d_offsets);
/* Host pointers, synchronous. */
int gd_send_queues(gd_handle* h, const uint32_t* silo, const uint8_t* route_status, const uint8_t* category,
                   const int64_t* ttl, uint32_t n, uint8_t* out_send_status, uint32_t* out_queue,
                   uint32_t* out_perm, uint32_t* out_offsets);
/* Dispatcher.AddressMessage then SendMessage (Dispatcher.cs:715-767 -> OutboundMessageQueue.cs:54-131):
 * gd_route_device, then the send stage on the route's own device outputs (silo, status), no host round
 * trip. */
int gd_route_send_device(gd_handle* h, const gd_key* d_keys, uint32_t n, const uint8_t* d_category,
                         const int64_t* d_ttl, uint32_t* d_silo, uint32_t* d_act, uint8_t* d_status,
                         uint8_t* d_send_status, uint32_t* d_queue, uint32_t* d_perm, uint32_t* d_offsets);
/* Host pointers, synchronous. */
int gd_route_send(gd_handle* h, const gd_key* keys, uint32_t n, const uint8_t* category, const int64_t* ttl,
                  uint32_t* out_silo, uint32_t* out_act, uint8_t* out_status, uint8_t* out_send_status,
                  uint32_t* out_queue, uint32_t* out_perm, uint32_t* out_offsets);

/* ---- placement of unregistered grains (Dispatcher.AddressMessageAsync's slow path) -------------
 * A message to a grain with no directory entry leaves the route GD_ROUTE_MISS; in the reference each such
 * message then takes four steps (Dispatcher.cs:742-767): PlacementDirectorsManager.SelectOrAddActivation
 * (PlacementDirectorsManager.cs:79-116) asks the grain class's placement director for a silo,
 * AddSingleActivation registers the new address, first wins (GrainDirectoryPartition.cs:304-326),
 * SetTargetPlacement writes it into the headers, and IsNewPlacement is set on the message that caused the
 * activation (Dispatcher.cs:753-767).  gd_route_place* does the four for a whole batch after the route:
 * one call leaves the batch addressed (and, in the *_bucket forms, bucketed), new grains included.
 *
 * Strategy, one byte a message (d_strategy) or default_strategy for all (d_strategy NULL):
 *   GD_PLACE_NONE   no placement: the message stays GD_ROUTE_MISS, as gd_route leaves it
 *   GD_PLACE_HASH   HashBasedPlacementDirector.cs:11-14: sorted_compatible[(uniform hash & 0x7fffffff)
 *                   % count], the compatible silos ordered by SiloAddress.CompareTo (gd_silo_compare)
 *   GD_PLACE_LOCAL  PreferLocalPlacementDirector.cs:17-26: gd_config.my_silo when the local silo is active
 *                   and compatible; otherwise the reference falls back to a random silo: here to
 *                   given_silo[i] when a given array is passed, else the message is skipped
 *   GD_PLACE_GIVEN  given_silo[i]: RandomPlacementDirector and ActivationCountPlacementDirector.cs:89-122
 *                   draw SafeRandom, so C# makes the choice and the library applies it (no given array:
 *                   skipped)
 * StatelessWorker grains (many activations, always local) are addressed by gd_workers_select*.
 *
 * Candidates: the messages that end the route GD_ROUTE_MISS and whose UniqueKey category is Grain (a Client
 * target is never placed, PlacementDirectorsManager.cs:85-93,108-109).  Every other message -- KeyExt grains,
 * system targets, the membership grain, GD_ROUTE_MULTI_ACT, hits -- keeps place status GD_PLACED_NONE and the
 * three outputs gd_route gives, bit for bit.  A candidate is GD_PLACED_SKIPPED, and stays GD_ROUTE_MISS, when
 * its strategy is NONE (or no known value), the compatible set is empty, LOCAL falls back without a given
 * silo, or the chosen silo is >= n_silos, not compatible, or not valid under gd_dir_set_valid_silos (the
 * IsValidSilo check of AddSingleActivation, GrainDirectoryPartition.cs:310).
 *
 * The batch equals the sequential order.  Walking the batch in order with c = 0: each non-skipped candidate
 * proposes activation act_base + c and increments c; if its grain is still absent it registers (proposal,
 * chosen silo) and leaves GD_ROUTE_OK with that address, GD_PLACED_NEW (the reference's IsNewPlacement); if
 * an earlier message of the batch registered the grain it leaves GD_ROUTE_OK with the winner's address,
 * GD_PLACED_JOINED.  Activation numbers are therefore sparse: a grain gets act_base + the rank of its first
 * placing message among the batch's placing candidates.  *out_n_proposed = the final c: the host advances
 * act_base by it.  A skipped message stays GD_ROUTE_MISS even when a later message of the batch places its
 * grain: its slow path in C# then finds the entry (the strategy is a property of the grain class, so a grain's
 * messages agree in practice).
 *
 * d_placed[n] receives the place status; d_new_idx (n entries, may be NULL) the ordered list of the
 * *out_n_new messages that created an entry: exactly the list the host creates its ActivationData from.
 * out_n_new and out_n_proposed are host words in every form: the device forms synchronise the handle's
 * stream to deliver them (once for a batch with no candidate; around the directory batch otherwise).
 * act_base + n_proposed reaching GD_ACT_MULTI fails with GD_EINVAL, nothing registered (the outputs are then
 * undefined).  The *_bucket forms run the bucketing (gd_bucket) on the final act array: a newly placed message
 * lands in its new activation's bucket, an act >= n_act in the unrouted bucket.  gd_stats.routed counts each
 * message once.  Inside a hipGraph capture, and on a handle in cache mode (gd_cache_configure: placement is
 * the directory owner's), the calls return GD_ESTATE without launching anything.
 *
 * gd_place_configure: the silo table (host pointers), compatible[s] != 0 = silo s can host the grains of the
 * batches that follow (NULL = all), local_active != 0 = the local silo's status is Active.  1 <= n_silos <=
 * 0xFFFE and silos non-NULL, else GD_EINVAL.  Sorts the compatible silos with gd_silo_compare; synchronises
 * the handle first (a batch in flight reads the table it was enqueued with); may be called again after a
 * membership change.  The batch calls return GD_ESTATE before it (a NULL handle has no configuration:
 * GD_ESTATE too, after the argument checks). */
#define GD_PLACE_NONE  0
#define GD_PLACE_HASH  1
#define GD_PLACE_LOCAL 2
#define GD_PLACE_GIVEN 3
#define GD_PLACED_NONE    0
#define GD_PLACED_NEW     1
#define GD_PLACED_JOINED  2
#define GD_PLACED_SKIPPED 3
int gd_place_configure(gd_handle* h, const gd_silo_addr* silos, uint32_t n_silos, const uint8_t* compatible,
                       int local_active);
int gd_route_place_device(gd_handle* h, const gd_key* d_keys, uint32_t n, const uint8_t* d_strategy,
                          int default_strategy, const uint32_t* d_given_silo, uint32_t act_base, uint32_t* d_silo,
                          uint32_t* d_act, uint8_t* d_status, uint8_t* d_placed, uint32_t* d_new_idx,
                          uint32_t* out_n_new, uint32_t* out_n_proposed);
/* Host pointers, synchronous. */
int gd_route_place(gd_handle* h, const gd_key* keys, uint32_t n, const uint8_t* strategy, int default_strategy,
                   const uint32_t* given_silo, uint32_t act_base, uint32_t* out_silo, uint32_t* out_act,
                   uint8_t* out_status, uint8_t* out_placed, uint32_t* out_new_idx, uint32_t* out_n_new,
                   uint32_t* out_n_proposed);
/* ... then the bucketing of the final act array: d_perm[n], d_offsets[n_act + 2] as gd_route_bucket_device. */
int gd_route_place_bucket_device(gd_handle* h, const gd_key* d_keys, uint32_t n, const uint8_t* d_strategy,
                                 int default_strategy, const uint32_t* d_given_silo, uint32_t act_base,
                                 uint32_t* d_silo, uint32_t* d_act, uint8_t* d_status, uint8_t* d_placed,
                                 uint32_t* d_new_idx, uint32_t* out_n_new, uint32_t* out_n_proposed, uint32_t n_act,
                                 uint32_t* d_perm, uint32_t* d_offsets);
/* Host pointers, synchronous. */
int gd_route_place_bucket(gd_handle* h, const gd_key* keys, uint32_t n, const uint8_t* strategy,
                          int default_strategy, const uint32_t* given_silo, uint32_t act_base, uint32_t* out_silo,
                          uint32_t* out_act, uint8_t* out_status, uint8_t* out_placed, uint32_t* out_new_idx,
                          uint32_t* out_n_new, uint32_t* out_n_proposed, uint32_t n_act, uint32_t* out_perm,
                          uint32_t* out_offsets);

/* ---- turn admission of a received batch (Dispatcher.ReceiveRequest) --------------------------------
 * What the closure IncomingMessageAgent enqueues does per message: Dispatcher.ReceiveMessage
 * (Core/Dispatcher.cs:75-123) -> ReceiveResponse (:238-254) or ReceiveRequest (:262-301) ->
 * ActivationMayAcceptRequest / CanInterleave (:313-336), HandleIncomingRequest (:399-424), EnqueueRequest
 * (:431-466), ProcessRequestToInvalidActivation (:468-484).  Under lock(activation), in arrival order, every
 * message of a received batch gets one outcome; gd_turns* gives all of them after gd_receive found the
 * activations, so the host takes no per-message lock.
 *
 * The batch model is gd_receive's: the InvokeWorkItem HandleIncomingRequest queues goes on the same
 * WorkItemGroup FIFO (WorkItemGroup.cs:174-201) as the batch's remaining closures, so no request of an
 * activation completes (ResetRunning never runs) between two receives of one batch.
 *
 * Per message: ctx and recv_status as gd_receive gave them, direction as for gd_receive (1 = Response, 0xFF =
 * absent = Request), ttl as for gd_send_queues (GD_TTL_NONE = no value), forward_count (Message.ForwardCount),
 * a GD_MSG_* flag byte, TargetActivation and SendingActivation.  Per context: a GD_CTX_* flag byte,
 * num_running (ActivationData.numRunning) and request_count = GetRequestCount() of the context once the agent
 * has enqueued the whole batch, i.e. gd_recv_limits.request_count[c] plus the messages gd_receive enqueued on
 * c (offsets[c + 1] - offsets[c]).
 *
 * Only messages with recv_status GD_RECV_ACTIVATION and ctx < n_ctx take part; every other message gets
 * GD_TURN_NONE and touches no state.  For a participating message of context c, with local copies of
 * num_running, has_running, running_ro and count (= request_count[c]), in arrival order:
 *   1. ttl has a value and ttl <= 0: GD_TURN_EXPIRED (:79-85, Message.cs:293-302).
 *   2. Response: GD_TURN_RESPONSE_DROPPED on an INVALID activation, else GD_TURN_RESPONSE.
 *   3. Request / OneWay on an INVALID activation: GD_TURN_FORWARD if forward_count < max_forward_count
 *      (MayForward, :627-630), else GD_TURN_REJECT_TRANSIENT (:563-568).
 *   4. accepted iff the state is VALID and (num_running == 0 or can_interleave), where can_interleave =
 *      ALWAYS_INTERLEAVE || !has_running || (running_ro && READ_ONLY) || (allow_call_chain_reentrancy &&
 *      TargetActivation == SendingActivation) || REENTRANT || MAY_INTERLEAVE (:326-336).
 *   5. accepted: GD_TURN_START; num_running++; if !has_running this message becomes Running and running_ro
 *      is its READ_ONLY flag (RecordRunning, ActivationData.cs:475-493).
 *   6. not accepted (EnqueueRequest): limit = the stateless-worker limit for a STATELESS_WORKER context, else
 *      hard_limit; limit > 0 && count > limit: GD_TURN_REJECT_OVERLOADED ("Overload2"); else STUCK:
 *      GD_TURN_STUCK; else GD_TURN_WAIT and count++ (the waiting list counts).
 *   7. count-- after any outcome (the closure's finally, IncomingMessageAgent.cs:184-187).
 * Outputs: d_turn[n]; d_num_running_out[n_ctx]; d_running_idx[n_ctx] = the batch index of the message that
 * became Running, else 0xFFFFFFFF; d_start_idx[n] holds the *d_n_start START messages in arrival order (the
 * InvokeWorkItems to queue; d_n_start is a device word in the *_device forms, nothing is read back);
 * d_wait_perm[n] / d_wait_offsets[n_ctx + 2] = the stable bucketing (gd_bucket's layout) of the WAIT messages
 * by context, every other message in the trailing bucket n_ctx: bucket c is what is appended to context c's
 * waiting list.
 *
 * Optional arrays: recv_status, direction, ttl, forward_count and msg_flags may be NULL (all-activation,
 * Request, no TTL, 0, 0).  The two activation key arrays are both given or both NULL (one alone: GD_EINVAL);
 * in the fused form the sending array alone may be NULL.  start_idx with n_start, and wait_perm with
 * wait_offsets, are each both or neither.  state, d_turn (n > 0), and with n_ctx > 0 ctx_flags, num_running,
 * d_num_running_out and d_running_idx are required; request_count is required when a limit is > 0.  n == 0 is
 * valid (the context outputs and list heads are still written).  n <= 2^31.  The calls are enqueue-only on the
 * handle's stream but return GD_ESTATE inside a hipGraph capture, as gd_route_place does (the bucketing they
 * reuse times its variants).
 *
 * Left to C#: deadlock detection (:277-293, off by default), the interface-version check of
 * HandleIncomingRequest (:403-410), logging (TryRescheduleCollection, :118: gd_collect_touch*), and the cross-cluster return in
 * TryForwardRequest.  The frame-fed form is gd_receive_turns_frames* (below): the decoder gives the read-only /
 * interleave / TTL / forward-count headers through gd_frame_turn_fields, a second struct beside gd_frame_fields
 * (which keeps its layout: GD_ABI_VERSION stays 1). */
#define GD_TURN_NONE              0
#define GD_TURN_START             1
#define GD_TURN_WAIT              2
#define GD_TURN_REJECT_OVERLOADED 3
#define GD_TURN_STUCK             4
#define GD_TURN_FORWARD           5
#define GD_TURN_REJECT_TRANSIENT  6
#define GD_TURN_EXPIRED           7
#define GD_TURN_RESPONSE          8
#define GD_TURN_RESPONSE_DROPPED  9
#define GD_MSG_READ_ONLY          1u  /* Message.IsReadOnly                                       */
#define GD_MSG_ALWAYS_INTERLEAVE  2u  /* Message.IsAlwaysInterleave                               */
#define GD_MSG_MAY_INTERLEAVE     4u  /* the grain class's MayInterleave predicate said yes (user
                                         code, evaluated in C#: Catalog.cs:409-417)               */
#define GD_CTX_VALID              0u  /* ActivationState.Valid                                    */
#define GD_CTX_NOT_READY          1u  /* Create / Activating / Deactivating (3 reads the same)     */
#define GD_CTX_INVALID            2u
#define GD_CTX_STATE_MASK         3u
#define GD_CTX_HAS_RUNNING        4u  /* Running != null when the batch starts                    */
#define GD_CTX_RUNNING_READ_ONLY  8u  /* Running.IsReadOnly                                       */
#define GD_CTX_REENTRANT         16u  /* GrainTypeData.IsReentrant, with a live GrainInstance     */
#define GD_CTX_STATELESS_WORKER  32u
#define GD_CTX_STUCK             64u  /* deactivatingTime or currentRequestActiveTime > maxRequestProcessingTime
                                         by the host's clocks before the batch (ActivationData.cs:576-594) */
typedef struct gd_turn_state {
    const uint8_t*  ctx_flags;       /* [n_ctx]; device memory for the *_device entry points */
    const uint32_t* num_running;     /* [n_ctx] */
    const uint32_t* request_count;   /* [n_ctx] */
    int32_t  hard_limit;             /* MaxEnqueuedRequestsHardLimit; <= 0 = none */
    int32_t  hard_limit_stateless_worker;
    uint32_t max_forward_count;      /* SiloMessagingOptions.MaxForwardCount */
    int32_t  allow_call_chain_reentrancy;   /* SchedulingOptions.AllowCallChainReentrancy */
} gd_turn_state;
int gd_turns_device(gd_handle* h, const uint32_t* d_ctx, const uint8_t* d_recv_status, const uint8_t* d_direction,
                    const int64_t* d_ttl, const uint8_t* d_forward_count, const uint8_t* d_msg_flags,
                    const gd_key* d_target_activation, const gd_key* d_sending_activation, uint32_t n, uint32_t n_ctx,
                    const gd_turn_state* state, uint8_t* d_turn, uint32_t* d_num_running_out, uint32_t* d_running_idx,
                    uint32_t* d_start_idx, uint32_t* d_n_start, uint32_t* d_wait_perm, uint32_t* d_wait_offsets);
/* Host pointers (state's arrays too; out_n_start a host word), synchronous. */
int gd_turns(gd_handle* h, const uint32_t* ctx, const uint8_t* recv_status, const uint8_t* direction,
             const int64_t* ttl, const uint8_t* forward_count, const uint8_t* msg_flags,
             const gd_key* target_activation, const gd_key* sending_activation, uint32_t n, uint32_t n_ctx,
             const gd_turn_state* state, uint8_t* out_turn, uint32_t* out_num_running, uint32_t* out_running_idx,
             uint32_t* out_start_idx, uint32_t* out_n_start, uint32_t* out_wait_perm, uint32_t* out_wait_offsets);
/* IncomingMessageAgent.ReceiveMessage then Dispatcher.ReceiveMessage: gd_receive_device, then the turn stage on
 * its own device outputs (d_ctx, d_status), no host round trip.  recv_limits / d_perm / d_offsets as
 * gd_receive_device; the call-chain test compares d_target_activation with d_sending_activation (NULL: no
 * message matches). */
int gd_receive_turns_device(gd_handle* h, const gd_key* d_target_grain, const gd_key* d_target_activation,
                            const uint8_t* d_direction, uint32_t n, uint32_t n_ctx, const gd_recv_limits* recv_limits,
                            uint32_t* d_ctx, uint8_t* d_status, uint32_t* d_perm, uint32_t* d_offsets,
                            const int64_t* d_ttl, const uint8_t* d_forward_count, const uint8_t* d_msg_flags,
                            const gd_key* d_sending_activation, const gd_turn_state* state, uint8_t* d_turn,
                            uint32_t* d_num_running_out, uint32_t* d_running_idx, uint32_t* d_start_idx,
                            uint32_t* d_n_start, uint32_t* d_wait_perm, uint32_t* d_wait_offsets);

/* ---- turn headers from the receive buffer ---------------------------------------------
 * The headers the turn stage and the callback table read, out of the same walk as gd_decode_frames
 * (HeadersContainer.Deserializer, Message.cs:1247-1356): one pass over the frames, one staging of each frame's
 * window.  n entries each; any pointer may be NULL (the field is not stored).
 *   - a bool is true iff its byte is SerializationTokenType.True (ReadBool, :1358-1361); any other byte, and a
 *     header bit set with a False token, reads 0.  The IS_NEW_PLACEMENT / IS_UNORDERED bytes are skipped.
 *   - a GD_FRAME_MALFORMED frame, and a GD_FRAME_FALLBACK one whose mask has CacheInvalidationHeader or
 *     RequestContext, has the absent value in every field (as it has zero keys); a frame that is FALLBACK only
 *     for its TargetObserver has all of them decoded (they precede it on the wire).
 *   - a present TimeToLive of TimeSpan.MaxValue equals GD_TTL_NONE: both mean "never expires", so the turn
 *     stage treats them alike.
 *   - ForwardCount is clamped to [0, 255] (gd_turns' byte); the reference never writes a negative one, which
 *     reads 0. */
typedef struct gd_frame_turn_fields {
    int64_t* ttl;             /* TimeToLive as written (TimeSpan ticks); GD_TTL_NONE when absent       */
    uint8_t* forward_count;   /* ForwardCount clamped to [0, 255]; 0 when absent                        */
    uint8_t* msg_flags;       /* GD_MSG_READ_ONLY | GD_MSG_ALWAYS_INTERLEAVE from the two bool tokens   */
    uint8_t* result;          /* Message.ResponseTypes byte; 0 when absent                              */
    uint8_t* rejection_type;  /* Message.RejectionTypes byte; 0 when absent                             */
    int32_t* resend_count;    /* 0 when absent                                                          */
} gd_frame_turn_fields;
/* gd_decode_frames* with the turn headers.  d_turn_out NULL (or all of its pointers NULL): exactly
 * gd_decode_frames*.  d_out->flags and d_out->target_grain stay required.  Device form: enqueue only. */
int gd_decode_frames_turn_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                                 uint32_t n, const gd_frame_fields* d_out, const gd_frame_turn_fields* d_turn_out);
/* Host pointers; synchronous. */
int gd_decode_frames_turn(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                          const gd_frame_fields* out, const gd_frame_turn_fields* turn_out);
/* Receive buffer -> decode -> IncomingMessageAgent.ReceiveMessage -> Dispatcher.ReceiveRequest with no host round
 * trip: gd_receive_frames_device, then the turn stage on its outputs and on the decoded direction, ttl, forward
 * count, flags, TargetActivation and SendingActivation (the call-chain test compares the decoded two).
 *   buffer .. d_offsets      as gd_receive_frames_device; d_out may be NULL (a non-NULL one needs flags and
 *                            target_grain), and names the decoded fields the caller wants back
 *   d_turn_out               may be NULL; names the turn headers the caller wants back, as the wire has them
 *                            (before ttl_age_ticks and d_msg_flags_or).  What is not asked for is decoded into
 *                            scratch of the handle
 *   ttl_age_ticks >= 0       Message.TimeToLive's getter is _timeToLive - (UtcNow - _localCreationTime)
 *                            (Message.cs:992-1002): the turn stage reads wire ttl - ttl_age_ticks for a ttl
 *                            with a value, saturating at INT64_MIN; GD_TTL_NONE stays.  < 0: GD_EINVAL
 *   d_msg_flags_or           NULL, or one GD_MSG_* byte a message OR-ed into the decoded flags: where C# puts
 *                            GD_MSG_MAY_INTERLEAVE (user code)
 *   state .. d_wait_offsets  as gd_receive_turns_device (state->request_count as described there)
 * A frame gd_receive_frames leaves GD_RECV_UNDECODED gets GD_TURN_NONE and touches no state.  Enqueue-only, but
 * GD_ESTATE inside a hipGraph capture, as gd_receive_turns_device. */
int gd_receive_turns_frames_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                                   uint32_t n, uint32_t n_ctx, const gd_recv_limits* recv_limits,
                                   const gd_frame_fields* d_out, const gd_frame_turn_fields* d_turn_out,
                                   uint32_t* d_ctx, uint8_t* d_status, uint32_t* d_perm, uint32_t* d_offsets,
                                   int64_t ttl_age_ticks, const uint8_t* d_msg_flags_or, const gd_turn_state* state,
                                   uint8_t* d_turn, uint32_t* d_num_running_out, uint32_t* d_running_idx,
                                   uint32_t* d_start_idx, uint32_t* d_n_start, uint32_t* d_wait_perm,
                                   uint32_t* d_wait_offsets);
/* Host pointers (state's and recv_limits' arrays too; out_n_start a host word); synchronous. */
int gd_receive_turns_frames(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                            uint32_t n_ctx, const gd_recv_limits* recv_limits, const gd_frame_fields* out,
                            const gd_frame_turn_fields* turn_out, uint32_t* out_ctx, uint8_t* out_status,
                            uint32_t* out_perm, uint32_t* out_offsets, int64_t ttl_age_ticks,
                            const uint8_t* msg_flags_or, const gd_turn_state* state, uint8_t* out_turn,
                            uint32_t* out_num_running, uint32_t* out_running_idx, uint32_t* out_start_idx,
                            uint32_t* out_n_start, uint32_t* out_wait_perm, uint32_t* out_wait_offsets);

/* ---- turn completion and message pump (Dispatcher.OnActivationCompletedRequest) ---------------------
 * The other half of the turn cycle: InvokeWorkItem.Execute's continuation (Scheduler/InvokeWorkItem.cs:50-55,
 * 62-63) calls Dispatcher.OnActivationCompletedRequest (Core/Dispatcher.cs:822-843) = ActivationData.
 * ResetRunning (Catalog/ActivationData.cs:495-514), then RunMessagePump (Core/Dispatcher.cs:845-874), which
 * takes messages off the activation's waiting list (PeekNextWaitingMessage / DequeueNextWaitingMessage,
 * ActivationData.cs:662-672) while ActivationMayAcceptRequest (:313-336) accepts the head, and starts each
 * (HandleIncomingRequest -> RecordRunning, ActivationData.cs:475-493).  gd_turns_complete* does this for a batch
 * of completions under the per-activation words gd_turns* already reads and writes (num_running,
 * GD_CTX_HAS_RUNNING, GD_CTX_RUNNING_READ_ONLY), so the host takes no lock per completed request.
 *
 * Per completion i, in arrival order: done_ctx[i], the activation's context as in gd_turns, and done_flags[i]
 * (the array may be NULL = all 0): GD_DONE_IS_RUNNING -- the completed message is the activation's Running as
 * of the batch start (message.Equals(Running)); GD_DONE_PUMP_ONLY -- no request completed, this is the bare
 * RunMessagePump Catalog.cs:1146-1158 makes when an activation turns Valid (step 1 is skipped).
 * Per context: ctx_flags[n_ctx] (GD_CTX_*) and num_running[n_ctx], read and written as two's-complement int32
 * in the uint32_t array (numRunning is an int; IsCurrentlyExecuting is numRunning > 0, :697-703).
 * The waiting lists are one CSR, gd_wait_list: context c's list is positions [offsets[c], offsets[c + 1]) in
 * FIFO order; msg[p] is the host's handle of the message (never interpreted here); flags[p] is a GD_MSG_* byte,
 * with GD_MSG_CALL_CHAIN = TargetActivation == SendingActivation with AllowCallChainReentrancy on when the
 * message was queued (read by these calls only).
 *
 * A completion with done_ctx[i] >= n_ctx takes no part (n_started_by[i] = 0).  For each other completion of
 * context c, in arrival order, with locals nr (int32), R in {none, X, a waiting position} (X = the batch-start
 * Running, present iff HAS_RUNNING, ro(X) = RUNNING_READ_ONLY), the list head p (from offsets[c]), event = 0:
 *   1. unless PUMP_ONLY (ResetRunning): nr -= 1; nr == 0: event |= GD_PUMP_BECAME_IDLE (becameIdle,
 *      TryRescheduleCollection, RunOnInactive: C#'s).  R == X and IS_RUNNING: R = none, event |=
 *      GD_PUMP_RUNNING_CLEARED.  R == none stays none; a message started in this batch never equals a
 *      completion of this batch.
 *   2. state != GD_CTX_VALID: next completion (:858).
 *   3. while p < offsets[c + 1]: f = flags[p]; accepted iff nr <= 0 || (f & ALWAYS_INTERLEAVE) || R == none ||
 *      (ro(R) && (f & READ_ONLY)) || (f & CALL_CHAIN) || (ctx_flags[c] & REENTRANT) || (f & MAY_INTERLEAVE);
 *      not accepted: stop.  Accepted (DequeueNextWaitingMessage, RecordRunning): nr += 1; if R == none: R = p,
 *      ro(R) = f & READ_ONLY, event |= GD_PUMP_RUNNING_SET; p is a start triggered by completion i; p += 1.
 * Outputs per context (a context with no taking-part completion: its inputs copied, 0 dequeued, no event):
 * num_running_out[c]; ctx_flags_out[c] = the input byte with HAS_RUNNING / RUNNING_READ_ONLY rewritten from R;
 * n_dequeued[c] = p - offsets[c] (the started messages of c are exactly that prefix of its list);
 * running_pos[c] = the waiting position that is Running at the end, else 0xFFFFFFFF; event[c].
 * Per completion and batch: n_started_by[i]; start_pos[0 .. *n_start) = all started waiting positions in the
 * order the sequential loop would have queued their InvokeWorkItems: by triggering completion, then FIFO
 * (*n_start a device word in the device form).  start_pos has wait_cap entries; the caller promises
 * offsets[n_ctx] <= wait_cap (the device form also reads no list position at or past wait_cap).
 *
 * One answer per batch is the sequential answer: a turn started by this batch's pump is an InvokeWorkItem
 * handed back to the host, so it completes in a later batch; waiting lists do not grow inside the batch; and
 * activations do not interact.  nr <= 0 with R != none is an inconsistent activation and is followed
 * literally, as gd_turns follows HAS_RUNNING with num_running == 0.  (|num_running| + list length < 2^31.)
 *
 * d_n_started_by, and d_start_pos with d_n_start, are optional (the latter two both or neither: GD_EINVAL).
 * wait, and with n_ctx > 0 wait->offsets and the context arrays, are required; wait->flags when wait_cap > 0.
 * n_done == 0 and n_ctx == 0 are valid (context outputs are still written).  n_done <= 2^31.  Enqueue-only on
 * the handle's stream; GD_ESTATE inside a hipGraph capture, as gd_turns_device (it reuses the bucketing).
 *
 * Left to C#: RunningRequestsSenders, the interface-version check of HandleIncomingRequest, RunOnInactive
 * (reported through GD_PUMP_BECAME_IDLE), logging.  (becameIdle and ResetRunning's TryRescheduleCollection:
 * gd_collect_idle* takes d_event as it is.) */
#define GD_MSG_CALL_CHAIN         8u
#define GD_DONE_IS_RUNNING        1u
#define GD_DONE_PUMP_ONLY         2u
#define GD_PUMP_BECAME_IDLE       1u
#define GD_PUMP_RUNNING_CLEARED   2u
#define GD_PUMP_RUNNING_SET       4u
typedef struct gd_wait_list {
    const uint32_t* offsets;   /* [n_ctx + 1]; device memory for the *_device entry points */
    const uint32_t* msg;       /* [offsets[n_ctx]] */
    const uint8_t*  flags;     /* [offsets[n_ctx]] */
} gd_wait_list;
int gd_turns_complete_device(gd_handle* h, const uint32_t* d_done_ctx, const uint8_t* d_done_flags, uint32_t n_done,
                             uint32_t n_ctx, const uint8_t* d_ctx_flags, const uint32_t* d_num_running,
                             const gd_wait_list* wait, uint32_t wait_cap, uint8_t* d_ctx_flags_out,
                             uint32_t* d_num_running_out, uint32_t* d_n_dequeued, uint32_t* d_running_pos,
                             uint8_t* d_event, uint32_t* d_n_started_by, uint32_t* d_start_pos, uint32_t* d_n_start);
/* Host pointers (wait's arrays too; out_n_start a host word), synchronous.  wait_cap >= offsets[n_ctx], else
 * GD_EINVAL. */
int gd_turns_complete(gd_handle* h, const uint32_t* done_ctx, const uint8_t* done_flags, uint32_t n_done,
                      uint32_t n_ctx, const uint8_t* ctx_flags, const uint32_t* num_running, const gd_wait_list* wait,
                      uint32_t wait_cap, uint8_t* out_ctx_flags, uint32_t* out_num_running, uint32_t* out_n_dequeued,
                      uint32_t* out_running_pos, uint8_t* out_event, uint32_t* out_n_started_by,
                      uint32_t* out_start_pos, uint32_t* out_n_start);
/* Keeps the CSR between steps: for every context the undequeued rest of its old list (old_list NULL or
 * old_list->offsets NULL = no old list; d_n_dequeued NULL = nothing dequeued; a count past the list's length
 * reads as the length), then bucket c of a gd_turns result (wait_perm[n], wait_offsets[n_ctx + 2]), both in
 * order.  Batch message i gets msg d_msg_id[i] (NULL: id_base + i) and flags d_msg_flags[i] (NULL: 0), plus
 * GD_MSG_CALL_CHAIN when allow_call_chain_reentrancy and its two activation keys are equal (the key arrays are
 * both given or both NULL).  d_offsets_out[n_ctx + 1] is always written; d_msg_out / d_flags_out have cap
 * entries and nothing is written at or past cap; *d_total = the entries needed (the caller compares it with cap
 * later; total < 2^32).  The outputs may not alias the inputs.  Enqueue-only on the handle's stream. */
int gd_wait_list_merge_device(gd_handle* h, const gd_wait_list* old_list, const uint32_t* d_n_dequeued, uint32_t n_ctx,
                              const uint32_t* d_wait_perm, const uint32_t* d_wait_offsets, uint32_t n,
                              const uint32_t* d_msg_id, uint32_t id_base, const uint8_t* d_msg_flags,
                              const gd_key* d_target_activation, const gd_key* d_sending_activation,
                              int allow_call_chain_reentrancy, uint32_t cap, uint32_t* d_offsets_out,
                              uint32_t* d_msg_out, uint8_t* d_flags_out, uint32_t* d_total);
/* Host pointers, synchronous; out_total a host word. */
int gd_wait_list_merge(gd_handle* h, const gd_wait_list* old_list, const uint32_t* n_dequeued, uint32_t n_ctx,
                       const uint32_t* wait_perm, const uint32_t* wait_offsets, uint32_t n, const uint32_t* msg_id,
                       uint32_t id_base, const uint8_t* msg_flags, const gd_key* target_activation,
                       const gd_key* sending_activation, int allow_call_chain_reentrancy, uint32_t cap,
                       uint32_t* out_offsets, uint32_t* out_msg, uint8_t* out_flags, uint32_t* out_total);

/* ---- activation collector (Catalog/ActivationCollector.cs, the whole file) ---------------------------
 * The idle tickets of the activations, the periodic stale scan and the condemned list that feeds
 * Catalog.DeactivateActivations -> gd_dir_unregister_device / gd_actdir_remove.  The reference keeps a
 * ConcurrentDictionary<DateTime, Bucket> of ConcurrentDictionary<ActivationId, ActivationData> and takes
 * lock(activation) per message (TryRescheduleCollection: Core/Dispatcher.cs:116-119, ActivationData.cs:500-507).
 * Here the collector is two words and a flag byte per context, caller-owned and updated in place (gd_collect_state;
 * device memory in the *_device forms), and two words on the handle: quantum and nextTicket.
 *
 * The invariant that replaces the dictionaries: context c is in bucket ticket[c] iff
 *     ticket[c] != 0 && !(flags[c] & GD_COL_CANCELLED) && ticket[c] >= nextTicket.
 * (tests/test_collect_ref.py holds it against a literal dictionary transcription after every step.)
 *
 * All times are DateTime.Ticks as int64 (0 < ticks < 2^62); DateTime.UtcNow is the call's `now`, also where the
 * reference reads the clock twice in one call.  roundup(t) = ((t - 1) / quantum + 1) * quantum
 * (MakeTicketFromDateTime, :368-377).  A batch gives the results of its items taken one by one in array order.
 *
 * gd_collect_configure(quantum_ticks, now): quantum and nextTicket = roundup(now) (:33-37); quantum_ticks <= 0 is
 *   GD_EINVAL.  Every other gd_collect_* call returns GD_ESTATE before it.  gd_collect_next_ticket reads
 *   nextTicket.  nextTicket lives on the host side of the handle: the device forms advance it when they enqueue
 *   (it is a function of `now` alone) and hand the old value to the kernel, so nothing is read back.
 * schedule = ScheduleCollection (:83-108) per ctx[i], checks in the reference's order: ctx[i] >= n_ctx
 *   GD_COL_OUT_OF_RANGE; exempt GD_COL_SKIPPED_EXEMPT; age_limit 0 GD_COL_SKIPPED_NO_LIMIT; age_limit < quantum
 *   GD_COL_THROWS_TIMEOUT (:381); t = roundup(now + age_limit) < nextTicket GD_COL_THROWS_EARLY (:372); ticket != 0
 *   GD_COL_THROWS_TICKETED (:101); else ticket = t, CANCELLED cleared (Add, :393), GD_COL_SCHEDULED.  Duplicates of
 *   a context: the first decides; later ones get THROWS_TICKETED if it was scheduled, else its status.
 * cancel = TryCancelCollection (:110-126): 1 iff not exempt, ticket != 0, ticket >= nextTicket and not CANCELLED;
 *   then CANCELLED is set and the ticket kept (Bucket.TryRemove).  Duplicates: the first gets 1, later ones 0.
 * touch = the Dispatcher.cs:116-119 site, fed by gd_receive*'s d_ctx and gd_turns*' turn bytes as they are.
 *   Message i takes part iff ctx[i] < n_ctx, turn[i] is one of GD_TURN_START, WAIT, REJECT_OVERLOADED, STUCK,
 *   FORWARD, REJECT_TRANSIENT (a non-expired Request / OneWay that reached ReceiveRequest; NONE, EXPIRED, RESPONSE
 *   and RESPONSE_DROPPED are out; turn NULL = every message) and ctx_flags[ctx[i]]'s state bits are GD_CTX_VALID.
 *   Then TryRescheduleCollection (:128-164), literally: exempt GD_COL_FALSE; ticket == 0 FALSE; ticket % quantum
 *   != 0 GD_COL_THROWS, state unchanged; ticket < nextTicket: ticket = 0, FALSE; age_limit < quantum THROWS;
 *   t = roundup(now + age_limit) < nextTicket THROWS (:372 again; now far behind nextTicket); t == ticket
 *   GD_COL_TRUE; CANCELLED: ticket = 0, FALSE; else ticket = t, TRUE.  A message that takes no part:
 *   GD_COL_NO_PART.  At one `now` the rule is idempotent on a context, so duplicates need no election: every
 *   occurrence gets the first's answer.
 * idle = the ResetRunning site, fed by gd_turns_complete*'s event bytes as they are: for every c with event[c] &
 *   GD_PUMP_BECAME_IDLE: became_idle[c] = now, then touch's rule (exempt: FALSE).  out_ok[n_ctx] optional, NO_PART
 *   for the others.
 * scan_stale = ScanStale (:206-264).  With next0 = nextTicket: n_q = next0 > now ? 0 : (now - next0) / quantum + 1
 *   quanta are dequeued (:166-190) and nextTicket += n_q * quantum; n_q > 2^28 is GD_EINVAL with nothing changed.
 *   Context c is due iff it is in a bucket, ticket[c] <= now and (ticket[c] - next0) % quantum == 0.  For a due
 *   context CANCELLED is set (CancelAll) and ticket = 0, then (:219-259), in order:
 *     state != GD_CTX_VALID                       GD_COL_BAD_STATE   nothing
 *     keep_alive_until >= now                     GD_COL_KEPT_ALIVE  ScheduleCollection (schedule's rule at now)
 *     (int32)num_running > 0 or a waiting list    GD_COL_ACTIVE      ScheduleCollection
 *     now - became_idle < age_limit               GD_COL_NOT_STALE   ScheduleCollection
 *     otherwise                                   GD_COL_COLLECT     PrepareForDeactivation: the state bits become
 *                                                                    GD_CTX_NOT_READY, other bits kept; listed
 *   A verdict whose ScheduleCollection did not add (any status but SCHEDULED; an exception in the reference) gets
 *   | GD_COL_NOT_ADDED.  A context that is not due is untouched, verdict 0.  out_ctx[0 .. *out_n) = the condemned
 *   contexts in ascending ticket, then ascending context index.  The reference's order inside one bucket is a
 *   ConcurrentDictionary enumeration, so unspecified: this order is ours.  Entries at and past *out_n are
 *   unspecified (out_ctx has n_ctx entries); *out_n is a device word in the device form.  The device form is
 *   enqueue-only, but with n_q > 1 it orders the list by the bucketing, which times its variants: GD_ESTATE inside
 *   a hipGraph capture, with nothing changed; it then takes 4 * (n_q + 2) bytes of scratch.
 * scan_all = ScanAll (:271-325): every context in a bucket gets the same chain's verdict with no re-schedule, the
 *   last test being now - became_idle >= age_limit_ticks; GD_COL_COLLECT: CANCELLED set, the ticket kept
 *   (TryRemove, :306), the state bits GD_CTX_NOT_READY, listed in ascending context index.  nextTicket stays.
 * count_recent = GetNumRecentlyUsed (:58-81, DeploymentLoadPublisher.cs:93): the contexts in a bucket when
 *   shortest_age_limit == 0, else those with shortest_age_limit - (ticket - now) <= recency.
 *
 * ticket, became_idle, age_limit and flags are required when n_ctx > 0; keep_alive_until NULL = never kept alive;
 * wait_offsets NULL = no waiting lists; the out_status / out_cancelled / out_ok / out_verdict outputs may be NULL.
 * n == 0 and n_ctx == 0 are valid.  n <= 2^31.
 *
 * Left to C#: Debug_OnDecideToCollectActivation, the warnings, ToString, DelayDeactivation (the host writes
 * keep_alive_until), Catalog.DeactivateActivations and everything after the list. */
#define GD_COL_EXEMPT             1u  /* flags: IsExemptFromCollection (collector == null), host-set */
#define GD_COL_CANCELLED          2u  /* flags: collectionCancelledFlag */
#define GD_COL_SCHEDULED          0
#define GD_COL_OUT_OF_RANGE       1
#define GD_COL_SKIPPED_EXEMPT     2
#define GD_COL_SKIPPED_NO_LIMIT   3
#define GD_COL_THROWS_TIMEOUT     4
#define GD_COL_THROWS_EARLY       5
#define GD_COL_THROWS_TICKETED    6
#define GD_COL_FALSE              0
#define GD_COL_TRUE               1
#define GD_COL_THROWS             2
#define GD_COL_NO_PART            3
#define GD_COL_BAD_STATE          1
#define GD_COL_KEPT_ALIVE         2
#define GD_COL_ACTIVE             3
#define GD_COL_NOT_STALE          4
#define GD_COL_COLLECT            5
#define GD_COL_NOT_ADDED       0x80
typedef struct gd_collect_state {
    int64_t*       ticket;            /* CollectionTicket in ticks; 0 = default(DateTime)               */
    int64_t*       became_idle;       /* becameIdle                                                     */
    const int64_t* keep_alive_until;  /* keepAliveUntil (DelayDeactivation, host-written); NULL = never */
    const int64_t* age_limit;         /* CollectionAgeLimit ticks; 0 = off / not initialised            */
    uint8_t*       flags;             /* GD_COL_EXEMPT, GD_COL_CANCELLED                                */
} gd_collect_state;
int gd_collect_configure(gd_handle* h, int64_t quantum_ticks, int64_t now);
int gd_collect_next_ticket(gd_handle* h, int64_t* out);
int gd_collect_schedule_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint32_t* d_ctx,
                               uint32_t n, int64_t now, uint8_t* d_status);
int gd_collect_schedule(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint32_t* ctx, uint32_t n,
                        int64_t now, uint8_t* out_status);
int gd_collect_cancel_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint32_t* d_ctx,
                             uint32_t n, uint8_t* d_cancelled);
int gd_collect_cancel(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint32_t* ctx, uint32_t n,
                      uint8_t* out_cancelled);
int gd_collect_touch_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint8_t* d_ctx_flags,
                            const uint32_t* d_ctx, const uint8_t* d_turn, uint32_t n, int64_t now, uint8_t* d_ok);
int gd_collect_touch(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint8_t* ctx_flags,
                     const uint32_t* ctx, const uint8_t* turn, uint32_t n, int64_t now, uint8_t* out_ok);
int gd_collect_idle_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint8_t* d_event,
                           int64_t now, uint8_t* d_ok);
int gd_collect_idle(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, const uint8_t* event, int64_t now,
                    uint8_t* out_ok);
int gd_collect_scan_stale_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, uint8_t* d_ctx_flags,
                                 const uint32_t* d_num_running, const uint32_t* d_wait_offsets, int64_t now,
                                 uint32_t* d_out_ctx, uint32_t* d_out_n, uint8_t* d_verdict);
/* Host pointers (the state's arrays too, updated in place; out_n a host word), synchronous; so are the host forms
 * above and below. */
int gd_collect_scan_stale(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, uint8_t* ctx_flags,
                          const uint32_t* num_running, const uint32_t* wait_offsets, int64_t now, uint32_t* out_ctx,
                          uint32_t* out_n, uint8_t* out_verdict);
int gd_collect_scan_all_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, uint8_t* d_ctx_flags,
                               const uint32_t* d_num_running, const uint32_t* d_wait_offsets, int64_t now,
                               int64_t age_limit_ticks, uint32_t* d_out_ctx, uint32_t* d_out_n, uint8_t* d_verdict);
int gd_collect_scan_all(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, uint8_t* ctx_flags,
                        const uint32_t* num_running, const uint32_t* wait_offsets, int64_t now,
                        int64_t age_limit_ticks, uint32_t* out_ctx, uint32_t* out_n, uint8_t* out_verdict);
int gd_collect_count_recent_device(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, int64_t now,
                                   int64_t shortest_age_limit, int64_t recency, uint64_t* d_count);
int gd_collect_count_recent(gd_handle* h, const gd_collect_state* st, uint32_t n_ctx, int64_t now,
                            int64_t shortest_age_limit, int64_t recency, uint64_t* out_count);

/* ---- callback table (InsideRuntimeClient.callbacks: SendRequest's TryAdd to ReceiveResponse) ---------
 * The outstanding requests of a silo: InsideRuntimeClient.callbacks, ConcurrentDictionary<CorrelationId,
 * CallbackData> (Core/InsideRuntimeClient.cs), as one table per handle in device memory, keyed by the 64-bit
 * CorrelationId.  An entry holds the host's callback handle (u32, never interpreted here), the message's
 * ResendCount, its TargetSilo as a silo index (GD_CB_NO_SILO = not addressed) and the deadline of its response
 * timer (int64 ticks).  With it a send -> receive -> turn -> complete -> respond cycle takes no per-message
 * dictionary operation on the host.  Calls are serialised by the caller, like every table of the handle; a batch
 * gives the results of its messages taken one by one in array order.
 *
 * gd_callbacks_configure(capacity_hint, max_resend_count, resend_on_timeout, period_ticks): the first call
 * creates the table (a power of two >= max(capacity_hint, 64) slots); a later call changes the options
 * (MessagingOptions.MaxResendCount <= 255, ResendOnTimeout) and grows the table if the hint asks for more.
 * period_ticks = timeout / (MaxResendCount + 1) when ResendOnTimeout && MaxResendCount > 0, else unused
 * (CallbackData.StartTimer, Orleans.Core/Runtime/CallbackData.cs:80-85).  The other calls return GD_ESTATE
 * before it.  gd_callbacks_clear empties the table; gd_callbacks_count reads the live entries and the slots.
 * The table holds live entries and the tombstones of removed ones; when both pass 0.75 of the slots an add
 * rebuilds it on the stream, at the same capacity while the live entries fill at most half of it, else at double;
 * GD_EFULL only when that allocation fails.
 *
 * add = SendRequestMessage's callbacks.TryAdd(message.Id, callbackData) + StartTimer (:205-218), before the
 *   message is addressed: per i, if ids[i] is absent the entry {handles[i], deadlines[i], resend 0, no target} is
 *   added and out_added[i] = 1, else nothing changes and out_added[i] = 0 (in the table or earlier in the batch:
 *   the first add wins).  out_added may be NULL.
 * set_target = Message.TargetSilo once gd_route* has addressed the batch, kept for break_silo: per i, a present
 *   ids[i] gets target silo[i] (GD_CB_NO_SILO allowed: ResendMessageImpl clears it, Core/Dispatcher.cs:618-620;
 *   else < 0xFFFF) and out_found[i] = 1, an absent one out_found[i] = 0; the last of an id in the batch stands.
 * lookup: read-only; out_handle (0xFFFFFFFF absent), out_resend (0), out_silo (GD_CB_NO_SILO), out_found; each
 *   output may be NULL.
 * respond = Dispatcher.ReceiveResponse (Core/Dispatcher.cs:238-254) -> InsideRuntimeClient.ReceiveResponse
 *   (:569-627) -> CallbackData.DoCallback (CallbackData.cs:126-157).  Per message: id; result (0 Success, 1 Error,
 *   2 Rejection, Message.cs:89-94; NULL array = all Success); rejection_type (0 Transient, 1 Overloaded,
 *   2 DuplicateRequest, 3 Unrecoverable, 4 GatewayTooBusy, :96-103; read only for a rejection, NULL = Transient);
 *   flags (NULL = 0): GD_RESP_TARGET_NOT_ME = !TargetSilo.Matches(CurrentSilo), GD_RESP_HAS_CACHE_HEADER =
 *   CacheInvalidationHeader != null; turn (optional, the gd_turns* output byte): only messages with
 *   turn == GD_TURN_RESPONSE take part, the others get GD_CB_NONE, flags 0, handle 0xFFFFFFFF.
 *   Per participating message, in array order:
 *     1. Rejection and TARGET_NOT_ME: GD_CB_GATEWAY_BACK (Transport.SendMessage is the caller's), nothing else
 *        (:573-579).
 *     2. Rejection of type Transient or Unrecoverable without the cache header: out_flags |=
 *        GD_CB_INVALIDATE_CACHE (:590-600); the caller invalidates SendingAddress (gd_cache_remove).
 *     3. id not in the table: GD_CB_NO_CALLBACK (:610,622-626).
 *     4. found, Rejection and Transient, and resend_count < max_resend_count (Message.MayResend, Message.cs:346-349;
 *        Dispatcher.TryResendMessage, Core/Dispatcher.cs:581-589): resend_count += 1, the target becomes none,
 *        GD_CB_RESEND, out_handle = the entry's handle; the entry stays (CallbackData.cs:135-141).
 *     5. otherwise GD_CB_FIRE, out_handle = the entry's handle, the entry is removed (alreadyFired, unregister:
 *        CallbackData.cs:143-149, InsideRuntimeClient.cs:247-251).
 *   out_handle is 0xFFFFFFFF unless RESEND or FIRE.  fire_idx / n_fire (optional, both or neither): the FIRE
 *   messages in array order, the order callback(response, context) runs in; fire_idx has n entries.
 *   Closed form (ids do not interact): among an id's responses that reach rule 3 and find the entry at the batch
 *   start, with k = max(max_resend_count - resend_count, 0) and f = min(rank of the first that is not a transient
 *   rejection, k): rank < f RESEND, rank == f FIRE, rank > f NO_CALLBACK.
 * expire = the response timers: CallbackData.OnTimeout -> OnFail(isOnTimeout) (CallbackData.cs:97-109,179-212).
 *   Every entry with deadline <= now, one tick an entry a call: if resend_on_timeout && resend_count <
 *   max_resend_count: resend_count += 1, deadline += period_ticks, target none, kind GD_CB_RESEND; else it is
 *   removed, kind GD_CB_TIMEOUT.  out_id / out_handle / out_kind [0 .. *n_out), in no particular order (timers
 *   have none).  *n_out > cap: nothing was changed or listed (host form: GD_EINVAL; device form: the caller
 *   compares the device word with cap).
 * break_silo = BreakOutstandingMessagesToDeadSilo (InsideRuntimeClient.cs:726-735) -> OnTargetSiloFail
 *   (CallbackData.cs:111-124): the same for every entry whose target is `silo`, the deadline untouched, kind
 *   GD_CB_RESEND or GD_CB_SILO_FAILED.
 *
 * The *_device forms take device pointers (n_fire / n_out device words) and only enqueue on the handle's stream,
 * except that an add whose room cannot be told from the host's bound reads the counters back (GD_ESTATE inside a
 * hipGraph capture); they run a fixed number of gated passes: an add of new ids that did not settle in 12 claim
 * passes, or a respond with more than 6 transient rejections resent for one id in one batch, is reported as
 * GD_ETIMEOUT by the next synchronising gd_callbacks_* call.  The host forms are synchronous and return
 * GD_ESTATE inside a capture.  n <= 2^31; n == 0 is valid.
 *
 * Left to C#: TransactionInfo.Join, the statistics, the callback invocation itself, the actual resend
 * (ResendMessageImpl), logging.  Dispatcher.ReceiveResponse's TryDeliverToProxy (Core/Dispatcher.cs:250) is
 * gd_gateway_deliver (the gateway block below), run ahead of respond on the same batch. */
#define GD_CB_NONE            0
#define GD_CB_FIRE            1
#define GD_CB_RESEND          2
#define GD_CB_NO_CALLBACK     3
#define GD_CB_GATEWAY_BACK    4
#define GD_CB_TIMEOUT         5
#define GD_CB_SILO_FAILED     6
#define GD_CB_INVALIDATE_CACHE  1u           /* out_flags bit */
#define GD_RESP_TARGET_NOT_ME     1u
#define GD_RESP_HAS_CACHE_HEADER  2u
#define GD_CB_NO_SILO         0xFFFFFFFFu
int gd_callbacks_configure(gd_handle* h, uint64_t capacity_hint, uint32_t max_resend_count, int resend_on_timeout,
                           int64_t period_ticks);
int gd_callbacks_clear(gd_handle* h);
int gd_callbacks_count(gd_handle* h, uint64_t* out_live, uint64_t* out_capacity);
int gd_callbacks_add_device(gd_handle* h, const int64_t* d_ids, const uint32_t* d_handles, const int64_t* d_deadlines,
                            uint32_t n, uint8_t* d_out_added);
int gd_callbacks_add(gd_handle* h, const int64_t* ids, const uint32_t* handles, const int64_t* deadlines, uint32_t n,
                     uint8_t* out_added);
int gd_callbacks_set_target_device(gd_handle* h, const int64_t* d_ids, const uint32_t* d_silo, uint32_t n,
                                   uint8_t* d_out_found);
int gd_callbacks_set_target(gd_handle* h, const int64_t* ids, const uint32_t* silo, uint32_t n, uint8_t* out_found);
int gd_callbacks_lookup_device(gd_handle* h, const int64_t* d_ids, uint32_t n, uint32_t* d_out_handle,
                               uint32_t* d_out_resend, uint32_t* d_out_silo, uint8_t* d_out_found);
int gd_callbacks_lookup(gd_handle* h, const int64_t* ids, uint32_t n, uint32_t* out_handle, uint32_t* out_resend,
                        uint32_t* out_silo, uint8_t* out_found);
int gd_callbacks_respond_device(gd_handle* h, const int64_t* d_ids, const uint8_t* d_result,
                                const uint8_t* d_rejection_type, const uint8_t* d_flags, const uint8_t* d_turn,
                                uint32_t n, uint8_t* d_out_outcome, uint8_t* d_out_flags, uint32_t* d_out_handle,
                                uint32_t* d_fire_idx, uint32_t* d_n_fire);
int gd_callbacks_respond(gd_handle* h, const int64_t* ids, const uint8_t* result, const uint8_t* rejection_type,
                         const uint8_t* flags, const uint8_t* turn, uint32_t n, uint8_t* out_outcome,
                         uint8_t* out_flags, uint32_t* out_handle, uint32_t* fire_idx, uint32_t* n_fire);
int gd_callbacks_expire_device(gd_handle* h, int64_t now, uint32_t cap, int64_t* d_out_id, uint32_t* d_out_handle,
                               uint8_t* d_out_kind, uint32_t* d_n_out);
int gd_callbacks_expire(gd_handle* h, int64_t now, uint32_t cap, int64_t* out_id, uint32_t* out_handle,
                        uint8_t* out_kind, uint32_t* n_out);
int gd_callbacks_break_silo_device(gd_handle* h, uint32_t silo, uint32_t cap, int64_t* d_out_id, uint32_t* d_out_handle,
                                   uint8_t* d_out_kind, uint32_t* d_n_out);
int gd_callbacks_break_silo(gd_handle* h, uint32_t silo, uint32_t cap, int64_t* out_id, uint32_t* out_handle,
                            uint8_t* out_kind, uint32_t* n_out);

/* ---- gateway: client table, TryDeliverToProxy, reply routes, client ingress ---------------
 * What a client-facing silo does per message in Messaging/Gateway.cs and GatewayAcceptor.cs that is not socket
 * code, for a batch: Gateway.clients (ConcurrentDictionary<GrainId, ClientState>, Gateway.cs:265-306) and
 * ClientsReplyRoutingCache.clientRoutes (:340-383) as two open-addressing tables per handle in device memory,
 * both keyed by the client's 24-B GrainId, category Client (UniqueKey.Category 4; GrainId.cs:23).  A client
 * entry holds the host's ClientState handle (u32, never interpreted here), GatewaySenderNumber, the connected
 * flag (Socket != null), DisconnectedSince (int64 ticks, INT64_MAX while connected: RecordConnection sets
 * DateTime.MaxValue, :295-299) and PendingToSend.Count (u32).  A route holds the gateway silo index (GD_NO_SILO
 * allowed: a null SendingSilo) and the tick it was recorded at.  Ticks are DateTime ticks: differences of two of
 * them do not overflow.  Calls are serialised by the caller, like every table of the handle; a batch gives the
 * results of its messages taken one by one in array order.  Geo clients (category GeoClient, 7) carry a KeyExt
 * string in their identity: every call reports them with a status of its own and does not touch them.
 *
 * gd_gateway_configure(n_senders, client_drop_timeout, route_expiry, capacity_hint): the first call creates both
 *   tables (a power of two >= max(capacity_hint, 64) slots each); a later call changes the options and grows the
 *   tables if the hint asks for more.  1 <= n_senders <= 1,024 (senders.Length); changing it while clients are
 *   present is GD_EINVAL.  client_drop_timeout = MessagingOptions.ClientDropTimeout, route_expiry = 5 x
 *   ResponseTimeout (:349), both in ticks, >= 0.  The other calls return GD_ESTATE before it.
 *   gd_gateway_clear empties both tables and resets the round robin; gd_gateway_count reads the live clients, the
 *   live routes and the two capacities (each output may be NULL).  A table holds live entries and the tombstones
 *   of removed ones; when both pass 0.75 of the slots, open (clients) or deliver (routes) rebuilds it on the
 *   stream, at the same capacity while the live entries fill at most half of it, else at double.
 * open = RecordOpenedSocket (:117-147), in array order.  An absent id is inserted with handles[i], sender
 *   (next_round_robin + its rank among the batch's new ids) % n_senders (:136-138), connected, pending 0:
 *   out_new = 1.  A present id -- in the table, or first seen earlier in the batch -- is a reconnect: it becomes
 *   connected, DisconnectedSince = INT64_MAX, out_new = 0, out_handle = the stored handle, out_pending = its
 *   pending count, which becomes 0 (QueueRequest(clientState, null), :132: the drain; the host sends its own
 *   queue).  next_round_robin advances by the number of new ids.  A key that is not of category Client gets
 *   out_new = GD_GW_NOT_CLIENT, out_handle 0xFFFFFFFF, out_sender = n_senders, and is not touched.  Each output
 *   may be NULL.
 * close = RecordClosedSocket -> RecordDisconnection (:149-169, :286-293).  A present, connected id: connected = 0,
 *   DisconnectedSince = now, and with pending_left given pending = pending_left[i] (what the host still holds
 *   after a failed drain); out_found = 1.  A present, disconnected id is untouched (Socket == null returns),
 *   out_found = 1.  Absent (or not a Client key): out_found = 0.  Which socket is which client's (clientSockets)
 *   stays in C#.
 * drop = DropDisconnectedClients (:182-222): every entry with !connected && now - DisconnectedSince >=
 *   client_drop_timeout (ReadyToDrop, :301-305) is removed and listed in out_id / out_handle / out_pending
 *   [0 .. *n_out), in no particular order.  *n_out > cap: nothing was changed or listed (host form: GD_EINVAL;
 *   device form: the caller compares the device word with cap).
 * routes_expire = DropExpiredEntries (:369-382): removes every route with now - recorded >= route_expiry;
 *   *n_removed = how many.
 * lookup: read-only.  Clients: out_handle (0xFFFFFFFF absent), out_sender (n_senders), out_connected (0),
 *   out_since (0), out_pending (0), out_found; routes: out_route_silo (GD_NO_SILO), out_route_time (0),
 *   out_route_found.  Each output may be NULL.
 * deliver = TryDeliverToProxy (:229-250) behind OutboundMessageQueue.cs:65-80, plus what GatewaySender.Process
 *   (:401-475) then decides.  Per message: target_grain, sending_grain (array NULL: no sender is a client),
 *   sending_silo (array NULL: GD_NO_SILO), ttl (gd_send_queues' meaning; NULL: none expire); scalar now.
 *   Statuses, in the reference's order:
 *     GD_GW_EXPIRED      ttl != GD_TTL_NONE && ttl <= 0 (OutboundMessageQueue.cs:65 runs before the proxy check)
 *     GD_GW_GEO_CLIENT   the target is a geo client: left to C#
 *     GD_GW_NOT_PROXIED  the target is not a Client or not in the client table: TryDeliverToProxy returns false
 *     GD_GW_SEND         the client is present and connected (Process sends on its socket)
 *     GD_GW_PENDING      present and disconnected: Process enqueues on PendingToSend (:424-429): pending += 1
 *   Process's "unrecognised client" branch (:411-416) cannot occur: lookup and processing are one step here.
 *   For every message that found its client and whose sending_grain is of category Client, the route table gets
 *   sending_grain -> (sending_silo, now) (RecordClientRoute = AddOrUpdate, :352-356): the last such message of
 *   a grain in the batch stands.  A geo-client sender is not recorded.
 *   out_handle: the ClientState handle (0xFFFFFFFF unless SEND or PENDING); out_sender: the client's sender number
 *   (n_senders for every other status).  perm[n] + offsets[n_senders + 2] (optional, both or neither): the batch's
 *   indices grouped by sender, each sender's in batch order (AsynchQueueAgent is a FIFO); everything not SEND or
 *   PENDING in the trailing bucket n_senders; offsets[n_senders + 1] = n.  n == 0 fills offsets with zeros.
 * send_queues = the send stage with the proxy check in its place (OutboundMessageQueue.cs:54-131): gd_send_queues'
 *   rule (gd_send_configure first) with one status added, GD_SEND_PROXIED, decided after HELD and EXPIRED and
 *   before NO_SILO (:77).  A proxied message gets deliver's out_handle and side effects; out_queue = n_queues + 4 +
 *   its sender number.  Buckets: gd_send_queues' n_queues + 4 unchanged, then one per gateway sender:
 *   offsets[n_queues + n_senders + 5], the last entry n.  The result equals gd_gateway_deliver followed by
 *   gd_send_queues on the not-proxied rest.
 * ingress = GatewayAcceptor.HandleMessage (GatewayAcceptor.cs:88-141) for a batch received from clients; read-only
 *   on the tables.  Per message: target_grain, sending_grain (NULL: no sender is a client), direction (gd_receive's
 *   byte, 1 = Response; NULL: all Requests), ttl (NULL: none expire); scalar overloaded (overloadDetector.Overloaded).
 *     GD_GWIN_EXPIRED        (:91)
 *     GD_GWIN_TOO_BUSY       overloaded (:106-114): the rejection and its TryDeliverToProxy are the caller's
 *     GD_GWIN_GEO_CLIENT     sender and target both IsClient, a Response, and the target a geo client: TryToReroute's
 *                            lookup is left to C# (categories compared only; both kinds count as IsClient)
 *     GD_GWIN_DIRECT         sender and target both IsClient, a Response, and the route table holds the target with
 *                            a silo other than GD_NO_SILO (Gateway.cs:171-180): out_silo = it, the caller calls
 *                            SendMessage (:138-139).  A route found with GD_NO_SILO is a null gateway: it reroutes.
 *     GD_GWIN_SYSTEM_TARGET  rerouted and the target a system target (:126-130): out_silo = gd_config.my_silo
 *     GD_GWIN_REROUTE        address cleared (:122-124): the message goes to gd_route*
 *   out_silo is GD_NO_SILO unless DIRECT or SYSTEM_TARGET.  route_idx[n] + n_route (optional, both or neither): the
 *   REROUTE messages in array order; route_keys[n] (optional, with them): their 24-B target keys compacted in that
 *   order, for gd_route_device with no host step.
 *
 * The *_device forms take device pointers (n_out / n_removed / n_route device words) and only enqueue on the
 * handle's stream, except that an open or a deliver whose room cannot be told from the host's bound reads the
 * counters back (GD_ESTATE inside a hipGraph capture; the bound counts one new entry a message); they run 12 gated
 * claim passes, and a batch of new ids that did not settle in them is reported as GD_ETIMEOUT by the next
 * synchronising gd_gateway_* call.  The host forms are synchronous and return GD_ESTATE inside a capture.
 * n <= 2^31; n == 0 is valid.
 *
 * Left to C#: the sockets and clientSockets, the PendingToSend queues themselves and their batches, rewriting
 * TargetSilo = null / SendingSilo = gatewayAddress in the frame (:246-247; gd_encode_frames* takes the caller's
 * fields), HasMultiClusterNetwork's sender translation (GatewayAcceptor.cs:100-103), clientRegistrar, statistics,
 * logging. */
#define GD_GW_NOT_PROXIED  0
#define GD_GW_SEND         1
#define GD_GW_PENDING      2
#define GD_GW_EXPIRED      3
#define GD_GW_GEO_CLIENT   4
#define GD_GW_NOT_CLIENT   0xFF              /* open's out_new */
#define GD_GW_MAX_SENDERS  1024u
#define GD_SEND_PROXIED    7                 /* gd_gateway_send_queues' added send status */
#define GD_GWIN_REROUTE        0
#define GD_GWIN_DIRECT         1
#define GD_GWIN_SYSTEM_TARGET  2
#define GD_GWIN_EXPIRED        3
#define GD_GWIN_TOO_BUSY       4
#define GD_GWIN_GEO_CLIENT     5
int gd_gateway_configure(gd_handle* h, uint32_t n_senders, int64_t client_drop_timeout, int64_t route_expiry,
                         uint64_t capacity_hint);
int gd_gateway_clear(gd_handle* h);
int gd_gateway_count(gd_handle* h, uint64_t* out_clients, uint64_t* out_routes, uint64_t* out_client_capacity,
                     uint64_t* out_route_capacity);
int gd_gateway_open_device(gd_handle* h, const gd_key* d_ids, const uint32_t* d_handles, uint32_t n,
                           uint32_t* d_out_handle, uint32_t* d_out_sender, uint8_t* d_out_new, uint32_t* d_out_pending);
int gd_gateway_open(gd_handle* h, const gd_key* ids, const uint32_t* handles, uint32_t n, uint32_t* out_handle,
                    uint32_t* out_sender, uint8_t* out_new, uint32_t* out_pending);
int gd_gateway_close_device(gd_handle* h, const gd_key* d_ids, const uint32_t* d_pending_left, uint32_t n, int64_t now,
                            uint8_t* d_out_found);
int gd_gateway_close(gd_handle* h, const gd_key* ids, const uint32_t* pending_left, uint32_t n, int64_t now,
                     uint8_t* out_found);
int gd_gateway_drop_device(gd_handle* h, int64_t now, uint32_t cap, gd_key* d_out_id, uint32_t* d_out_handle,
                           uint32_t* d_out_pending, uint32_t* d_n_out);
int gd_gateway_drop(gd_handle* h, int64_t now, uint32_t cap, gd_key* out_id, uint32_t* out_handle,
                    uint32_t* out_pending, uint32_t* n_out);
int gd_gateway_routes_expire_device(gd_handle* h, int64_t now, uint32_t* d_n_removed);
int gd_gateway_routes_expire(gd_handle* h, int64_t now, uint32_t* n_removed);
int gd_gateway_lookup_device(gd_handle* h, const gd_key* d_ids, uint32_t n, uint32_t* d_out_handle,
                             uint32_t* d_out_sender, uint8_t* d_out_connected, int64_t* d_out_since,
                             uint32_t* d_out_pending, uint8_t* d_out_found, uint32_t* d_out_route_silo,
                             int64_t* d_out_route_time, uint8_t* d_out_route_found);
int gd_gateway_lookup(gd_handle* h, const gd_key* ids, uint32_t n, uint32_t* out_handle, uint32_t* out_sender,
                      uint8_t* out_connected, int64_t* out_since, uint32_t* out_pending, uint8_t* out_found,
                      uint32_t* out_route_silo, int64_t* out_route_time, uint8_t* out_route_found);
int gd_gateway_deliver_device(gd_handle* h, const gd_key* d_target_grain, const gd_key* d_sending_grain,
                              const uint32_t* d_sending_silo, const int64_t* d_ttl, uint32_t n, int64_t now,
                              uint8_t* d_out_status, uint32_t* d_out_handle, uint32_t* d_out_sender, uint32_t* d_perm,
                              uint32_t* d_offsets);
int gd_gateway_deliver(gd_handle* h, const gd_key* target_grain, const gd_key* sending_grain,
                       const uint32_t* sending_silo, const int64_t* ttl, uint32_t n, int64_t now, uint8_t* out_status,
                       uint32_t* out_handle, uint32_t* out_sender, uint32_t* out_perm, uint32_t* out_offsets);
int gd_gateway_send_queues_device(gd_handle* h, const gd_key* d_target_grain, const gd_key* d_sending_grain,
                                  const uint32_t* d_sending_silo, const uint32_t* d_silo,
                                  const uint8_t* d_route_status, const uint8_t* d_category, const int64_t* d_ttl,
                                  uint32_t n, int64_t now, uint8_t* d_send_status, uint32_t* d_queue,
                                  uint32_t* d_out_handle, uint32_t* d_perm, uint32_t* d_offsets);
int gd_gateway_send_queues(gd_handle* h, const gd_key* target_grain, const gd_key* sending_grain,
                           const uint32_t* sending_silo, const uint32_t* silo, const uint8_t* route_status,
                           const uint8_t* category, const int64_t* ttl, uint32_t n, int64_t now,
                           uint8_t* out_send_status, uint32_t* out_queue, uint32_t* out_handle, uint32_t* out_perm,
                           uint32_t* out_offsets);
int gd_gateway_ingress_device(gd_handle* h, const gd_key* d_target_grain, const gd_key* d_sending_grain,
                              const uint8_t* d_direction, const int64_t* d_ttl, uint32_t n, int overloaded,
                              uint8_t* d_out_status, uint32_t* d_out_silo, uint32_t* d_route_idx, uint32_t* d_n_route,
                              gd_key* d_route_keys);
int gd_gateway_ingress(gd_handle* h, const gd_key* target_grain, const gd_key* sending_grain, const uint8_t* direction,
                       const int64_t* ttl, uint32_t n, int overloaded, uint8_t* out_status, uint32_t* out_silo,
                       uint32_t* route_idx, uint32_t* n_route, gd_key* route_keys);

/* ---- stateless workers: worker sets, pick, grow, spread --------------------------------
 * A message to a grain class whose strategy is StatelessWorkerPlacement is addressed by
 * StatelessWorkerDirector.SelectActivationCore (Placement/StatelessWorkerDirector.cs:31-62): FindTargets copies the
 * grain's local activations under a lock (ActivationDirectory.cs:150-158), the first Valid and inactive one
 * (ActivationData.IsInactive, ActivationData.cs:689-703) takes the message (:46-53), else a new local activation is
 * made while fewer than MaxLocal exist (:26-29,61), else a random one is drawn (:55-59).  gd_workers_select* does
 * this for a batch over worker sets kept on the device, and its d_ctx feeds gd_turns_device directly.
 *
 * State: one table per handle, GrainId -> set = {count, max_local, the ctx list in List<ActivationData> order, at
 * most slot_capacity entries}.  gd_workers_configure(capacity = sets expected, slot_capacity, default_max_local):
 * 1 <= slot_capacity <= GD_WK_MAX_SLOT_CAPACITY and 1 <= default_max_local <= slot_capacity, else GD_EINVAL;
 * called again it may raise the capacity, and change slot_capacity only while no set exists.  The batch calls
 * return GD_ESTATE before it.  The table grows on its own.  The contexts of one set are distinct (the caller's
 * promise; 0xFFFFFFFF is no context).
 *
 * The batch model (a choice: one legal interleaving of the reference, not something it guarantees).  Messages are
 * addressed in batch order, and each is delivered (Dispatcher.ReceiveRequest) before the next is addressed.  So a
 * worker picked while inactive is executing for the rest of the batch, a worker the batch creates is in state
 * Create (not Valid) for the rest of the batch, and nothing completes inside the batch.  Per set at the batch
 * start: L[0..c) its list, m its MaxLocal, I the entries of L, in list order, with ctx < n_ctx, state
 * GD_CTX_VALID, (int32)num_running <= 0 and an empty waiting list (d_wait_offsets: gd_wait_list's offsets, NULL =
 * all empty); a = |I|, room = max(0, m - c), C = c + room.  The message whose stable rank among the batch's
 * messages of that set is k gets d_pick:
 *   GD_WK_IDLE    k < a: d_ctx = I[k].
 *   GD_WK_NEW     a <= k < a + room: d_ctx = ctx_base + g, g = the message's rank among the call's NEW messages
 *                 in batch order (dense); the library appends L[c + (k - a)] = d_ctx.
 *   GD_WK_RANDOM  otherwise: d_ctx = L'[r] of the final list L' (length C); r = 0 when C == 1 (the draw is not
 *                 read), else (int)(((double)d_draw[i] * (1.0 / 2147483647.0)) * (double)C): Random.Next(C) on
 *                 the internal sample C# got from random.Next() for this message.
 *   GD_WK_HELD    a RANDOM message with d_draw NULL or d_draw[i] >= 0x7FFFFFFF: left to C#, its rank consumed;
 *                 also a message whose max_local exceeds slot_capacity (it takes no part and creates nothing).
 *   GD_WK_NONE    the key's UniqueKey category is not Grain (the reference throws for clients, :33-34).
 * HELD and NONE give d_ctx 0xFFFFFFFF.  A message of a grain with no set creates it (c = 0) with m = its
 * d_max_local entry (int32; <= 0, or the array NULL = default_max_local); the first such message decides.
 * d_new_idx[0 .. n_new) lists the NEW messages in batch order (optional, with n_new: both or neither, else
 * GD_EINVAL); n_new is a device word in the device form.  ctx_base + n past GD_ACT_MULTI is GD_EINVAL (n_new <= n
 * is what the host knows before the batch runs).  With n_ctx > 0 the two context arrays are required.
 *
 * gd_workers_add*: RecordNewTarget (ActivationDirectory.cs:86-93) for a batch, appended in batch order, several
 * of one grain included; a grain with no set gets one with the item's max_local.  out_status: GD_WK_ADDED,
 * GD_WK_FULL (the list is at slot_capacity, or max_local > slot_capacity), GD_WK_NOT_GRAIN.
 * gd_workers_remove*: RemoveTarget's list.Remove (:116-147) per (grain, ctx) pair in batch order: the first
 * occurrence goes, the order of the rest is kept, a set left empty is removed; out_removed = 1 / 0.
 * gd_workers_lookup*: per key count, max_local and the list (n * slot_capacity words, the unused tail
 * 0xFFFFFFFF; each output optional); a grain with no set reads 0, 0, empty.
 *
 * The device forms are enqueue-only on the handle's stream while the host's bound (one new set a message since
 * the last read-back) leaves the table under load 0.75; past it a batch that may create sets reads its count of
 * set-less messages back, and grows the table when they need the room.  select and add run 12 gated claim
 * passes; a batch that did not settle in them is reported as GD_ETIMEOUT by the next synchronising gd_workers_*
 * call (its unsettled messages are HELD / FULL).  All three batch calls reuse the bucketing, so they return
 * GD_ESTATE inside a hipGraph capture, as gd_turns_device does, with nothing launched.  The host forms are
 * synchronous.  n <= 2^31; n == 0 is valid.
 *
 * Left to C#: the registration-time overshoot check and its PickRandom (Catalog.cs:1284-1293), re-routing of
 * queued messages when a worker deactivates, and the RNG itself (SafeRandom: the host passes what Next() gave). */
#define GD_WK_MAX_SLOT_CAPACITY 1024
#define GD_WK_NONE   0
#define GD_WK_IDLE   1
#define GD_WK_NEW    2
#define GD_WK_RANDOM 3
#define GD_WK_HELD   4
#define GD_WK_NOT_GRAIN 0            /* gd_workers_add's out_status */
#define GD_WK_ADDED     1
#define GD_WK_FULL      2
int gd_workers_configure(gd_handle* h, uint64_t capacity, uint32_t slot_capacity, uint32_t default_max_local);
int gd_workers_clear(gd_handle* h);
int gd_workers_count(gd_handle* h, uint64_t* out_sets, uint64_t* out_capacity);
int gd_workers_add_device(gd_handle* h, const gd_key* d_grains, const uint32_t* d_ctx, const int32_t* d_max_local,
                          uint32_t n, uint8_t* d_out_status);
int gd_workers_add(gd_handle* h, const gd_key* grains, const uint32_t* ctx, const int32_t* max_local, uint32_t n,
                   uint8_t* out_status);
int gd_workers_remove_device(gd_handle* h, const gd_key* d_grains, const uint32_t* d_ctx, uint32_t n,
                             uint8_t* d_out_removed);
int gd_workers_remove(gd_handle* h, const gd_key* grains, const uint32_t* ctx, uint32_t n, uint8_t* out_removed);
int gd_workers_lookup_device(gd_handle* h, const gd_key* d_grains, uint32_t n, uint32_t* d_out_count,
                             uint32_t* d_out_max_local, uint32_t* d_out_list);
int gd_workers_lookup(gd_handle* h, const gd_key* grains, uint32_t n, uint32_t* out_count, uint32_t* out_max_local,
                      uint32_t* out_list);
int gd_workers_select_device(gd_handle* h, const gd_key* d_grains, uint32_t n, const int32_t* d_max_local,
                             const uint32_t* d_draw, uint32_t ctx_base, uint32_t n_ctx, const uint8_t* d_ctx_flags,
                             const uint32_t* d_num_running, const uint32_t* d_wait_offsets, uint32_t* d_ctx,
                             uint8_t* d_pick, uint32_t* d_new_idx, uint32_t* d_n_new);
/* Host pointers (the context arrays too; n_new a host word), synchronous. */
int gd_workers_select(gd_handle* h, const gd_key* grains, uint32_t n, const int32_t* max_local, const uint32_t* draw,
                      uint32_t ctx_base, uint32_t n_ctx, const uint8_t* ctx_flags, const uint32_t* num_running,
                      const uint32_t* wait_offsets, uint32_t* out_ctx, uint8_t* out_pick, uint32_t* out_new_idx,
                      uint32_t* n_new);

/* ---- compact route: (class, N1) records in, packed routes out ---------------------------
 * A long-keyed grain's GrainId is {N0 = 0, N1 = the long key, TypeCodeData = one of the handle's few grain
 * classes} (GrainId.GetGrainId(typeCode, long), GrainId.cs:72-77): 16 of its 24 bytes are constant.  These calls
 * take such messages as records -- a class id (u8, the index into the handle's class table) and N1 (u32 or
 * u64, zero-extended) -- and give the routes packed: act u32, silo u16, status u8.  A message costs 4, 5, 8 or 9
 * bytes going up and 7 coming down (plus 4 of perm) instead of 24 and 9.
 *
 * gd_classes_set(type_code_data[n], n <= 256) replaces the handle's class table (n = 0 clears it); the class id
 * is the array index.  It synchronises the handle's stream.  gd_classes_get gives up to max entries back and
 * the table's size in *out_n.
 *
 * Input, structure-of-arrays: cls[n] (NULL: every message is class 0) and n1[n] of n1_width 4 (uint32_t) or 8
 * (uint64_t) bytes.  Output: out_act[n], out_silo16[n], out_status[n]; the bucket forms also perm[n] and
 * offsets[n_act + 2], exactly as gd_route_bucket gives them (misses in the trailing bucket).
 *
 * For each message the key is {0, n1[i], classes[cls[i]]} and (act, silo, status) are what gd_route* gives
 * for that key -- GD_ROUTE_OK, _MISS, _SYSTEM_TARGET, _MEMBERSHIP, _KEYEXT (a class of a KeyExt category; its
 * string never reaches these calls) and _MULTI_ACT -- in every ring mode, and in LocalLookup (cache) mode with
 * the same cache hits and LRU touches in the same batch order.  Two values are these calls' own:
 *   GD_NO_SILO16        GD_NO_SILO as 16 bits.
 *   GD_ROUTE_BAD_CLASS  cls[i] is not below the table's size: act = GD_NO_ACTIVATION, silo = GD_NO_SILO16; in
 *                       LocalLookup mode the message touches no cache entry and counts no access.
 * A silo index in 0xFFFF..0xFFFFFFFE does not fit: GD_NO_SILO16 is stored and the message counted.  The
 * directory, the cache and the ring hold silo indexes up to 0xFFFE, so only cfg.my_silo (system targets) and
 * cfg.seed_silo (the membership grain) can be that wide.  The host forms synchronise, bring every result down
 * and then return GD_EINVAL when the count is not zero; the device forms store the count in *d_wide (optional,
 * NULL allowed; zeroed by the call on the handle's stream).
 *
 * Errors: GD_EINVAL for an n1_width other than 4 or 8 and for null arguments; with n > 0, GD_ESTATE when no
 * class table is set (class 0 is absent, whether cls is NULL or not).  n = 0 is GD_OK and the bucket forms
 * write offsets.  Host forms: pinned buffers (gd_host_alloc) of at least two GD_OPT_HOST_CHUNK chunks take
 * gd_route_bucket's copy / route / copy pipeline over the record streams, anything else one copy each way. */
#define GD_NO_SILO16       0xFFFFu
#define GD_ROUTE_BAD_CLASS 8
int gd_classes_set(gd_handle* h, const uint64_t* type_code_data, uint32_t n);
int gd_classes_get(gd_handle* h, uint64_t* out_type_code_data, uint32_t max, uint32_t* out_n);
int gd_route_compact(gd_handle* h, const uint8_t* cls, const void* n1, uint32_t n1_width, uint32_t n, uint32_t* out_act,
                     uint16_t* out_silo16, uint8_t* out_status);
int gd_route_bucket_compact(gd_handle* h, const uint8_t* cls, const void* n1, uint32_t n1_width, uint32_t n,
                            uint32_t n_act, uint32_t* out_act, uint16_t* out_silo16, uint8_t* out_status,
                            uint32_t* out_perm, uint32_t* out_offsets);
/* Device pointers, on the handle's stream, no synchronisation (the bucketing as gd_route_bucket_device's:
 * on the bucket stream when one is set). */
int gd_route_compact_device(gd_handle* h, const uint8_t* d_cls, const void* d_n1, uint32_t n1_width, uint32_t n,
                            uint32_t* d_act, uint16_t* d_silo16, uint8_t* d_status, uint32_t* d_wide);
int gd_route_bucket_compact_device(gd_handle* h, const uint8_t* d_cls, const void* d_n1, uint32_t n1_width, uint32_t n,
                                   uint32_t n_act, uint32_t* d_act, uint16_t* d_silo16, uint8_t* d_status,
                                   uint32_t* d_perm, uint32_t* d_offsets, uint32_t* d_wide);

/* ---- per-kernel timing (cfg.flags & GD_CFG_KERNEL_TIMING) ----------------------- */
/* Up to max entries of {name, launches, total_ms} accumulated since the last reset. */
typedef struct gd_kernel_time {
    char     name[48];
    uint64_t launches;
    double   total_ms;
} gd_kernel_time;
int gd_kernel_times(gd_handle* h, gd_kernel_time* out, uint32_t max, uint32_t* out_n);
int gd_kernel_times_reset(gd_handle* h);
int gd_set_kernel_timing(gd_handle* h, int enable);   /* 0 off, 1 every launch, 2 stages only
                                                         ("stage:bucket": one event pair around each
                                                         bucketing, none between its kernels) */

/* ---- handle options (no reference counterpart: the reference has no device kernels) ------------
 * Round 4 replaces the library's GD_* environment switches: a host's behaviour no longer depends on
 * its environment, only on these calls.  Every option changes speed only, never results (the parity
 * tests run both sides of each one that changes a data layout); the defaults are the measured
 * winners.  Exchange options are per sender and may differ between ranks. */
#define GD_OPT_PROBE        1   /* route probe: 0 directory, 1 measured per launch kind (default),
                                   2 compact index in 64-B group reads, 3 compact index in 16-B slot reads,
                                   4 the 8-B index where the directory allows it (one type, N1 < 2^32,
                                   activation and silo numbers fitting a u32 together; else as 2) */
#define GD_OPT_BUCKET       2   /* bucketing: 0 LSD passes, 1 measured (default), 2 the two-level form
                                   wherever it applies (batches >= 2^20 messages, n_act < 2^28) */
#define GD_OPT_L2_SMALL     3   /* two-level three-pass form: ranges of at most this many messages are
                                   sorted one wave a range (default 1024) */
#define GD_OPT_STABLE_RANK  4   /* every bucketing form's in-wave rank: 1 ds_add_rtn, whose same-address
                                   lanes the hardware serves in lane order (default; gd_create checks that
                                   order on the device), 0 ballots -- stable by construction; a device
                                   failing the check gets 0 and refuses 1 */
#define GD_OPT_WIRE_HEADERS 5   /* exchange headers of one-type long-key batches: 0 24-B keys, 1 u64
                                   N1s, 2 u32 N1s when every N1 < 2^32 (default) */
#define GD_OPT_REGION_PROBE 6   /* exchange: (rank, region) partition + region-mapped owner probe: 0 (default) / 1 */
#define GD_OPT_IDX16        7   /* exchange at W > 1: 2-B origin indices on the wire: 1 (default) / 0 */
#define GD_OPT_HOST_CHUNK   8   /* host-pointer gd_route / gd_route_bucket: messages a pipelined chunk
                                   (default 2,097,152; 0 = one chunk, the serial copies) */
#define GD_OPT_MB_ZEROCOPY  9   /* micro-batches created after: I/O from / to pinned host memory: 1 (default)
                                   / 0 staged copies */
#define GD_OPT_MB_SPLIT     10  /* micro-batches created after: redundant sorters splitting the host stores (8) */
#define GD_OPT_MB_TRACE     11  /* micro-batches created after: per-phase timestamps printed at destroy (0) */
#define GD_OPT_L2_STAGED    12  /* two-level three-pass form: ranges of at most this many messages (and more
                                   than GD_OPT_L2_SMALL) sorted one workgroup a range, larger ones in 8K
                                   chunks over several workgroups (default 24,576, the staging capacity) */
#define GD_OPT_L2_MID       13  /* two-level three-pass form: ranges of at most this many messages (and more
                                   than GD_OPT_L2_SMALL) sorted by 512-thread workgroups, three a CU, the rest
                                   of the staged class by 1,024-thread ones (default 8,192, the 512-thread
                                   capacity; 0 = every staged range on the 1,024-thread sort) */
#define GD_OPT_B2_PERSIST   14  /* one-pass two-level form's MSD scatter: k = 1..8 persistent workgroups a
                                   CU, each loading its next tile under the current tile's write-out
                                   (default 2); 0 one workgroup a tile */
#define GD_OPT_B2_ORDER     15  /* that persistent scatter's tile order within its XCD's tile range: 0 strided
                                   (workgroup k takes tiles k, k + per, ...), 1 chunked (workgroup k takes a
                                   run of consecutive tiles, so one digit's runs of neighbouring tiles -- one
                                   128-B line between them -- leave one workgroup back to back; measured
                                   slower, profiles/r06_b2_order_ab.txt) */
#define GD_OPT_MB_POLL      16  /* micro-batches created after, zero-copy: a graph replay (gd_microbatch_run
                                   with use_graph) returns when the sort's workgroups have counted
                                   themselves done in pinned host memory (their stores fenced first)
                                   instead of waiting for the dispatch's completion signal; eager runs
                                   still synchronise the stream (measured faster): 1 (default) / 0 */
#define GD_OPT_FAN_BOUND    17  /* measurement: each fan-out route over the 8-B index is preceded by a launch
                                   of its memory traffic alone (k_fan_bound: the same expansion reads, one
                                   64-B index group read a message and the same result writes into scratch,
                                   no ring search, no walk), timed under its own name: 0 (default) / 1 */
#define GD_OPT_WALK_INVALIDATION 18 /* frames that carry a CacheInvalidationHeader (every request
                                   gd_forward_frames* forwards, and the answers to them): 0 (default) they go
                                   back to C# -- GD_FRAME_FALLBACK, GD_ENC_FALLBACK, GD_RSPST_FALLBACK; 1 the
                                   decoder (every gd_*_frames* call it feeds, gd_receive_activate_turns_frames*'
                                   IsNewPlacement walk included), gd_encode_frames* and gd_respond_frames* step
                                   over the field (GD_FRAME_INVALIDATION, and the two stages' contracts).  With 0
                                   the kernels launched are the ones without the walk, bit for bit */
int gd_option_set(gd_handle* h, int option, int64_t value);
int gd_option_get(const gd_handle* h, int option, int64_t* value);

/* ---- measured choices -------------------------------------------------------------------------
 * With GD_OPT_PROBE / GD_OPT_BUCKET at 1 the library times its interchangeable variants on the first
 * launches of each launch kind and size class (HIP events, read without a stream sync) and keeps the
 * fastest per message.  These calls let a host see, pin and share those choices, so that performance
 * is deterministic: pinned choices run from the first launch; gd_tune_agree makes every rank of the
 * communicator run the same variant. */
#define GD_TUNE_PROBE_KEYS   0  /* k_route over 24-B keys: 0 index groups, 1 directory, 2 index slots,
                                   3 the 8-B index (when the directory allows it) */
#define GD_TUNE_PROBE_N1     1  /* the exchange owner's probe over received N1s: same variants (0..3) */
#define GD_TUNE_PROBE_FANOUT 2  /* k_fan_route: 0 index groups, 1 directory, 2 the 8-B index */
#define GD_TUNE_PROBE_NODES  3  /* the sharded fan-out owner's probe: 0 index groups, 1 directory, 2 the 8-B index */
#define GD_TUNE_BUCKET       4  /* bucketing: 0 LSD passes, 1 the two-level form */
#define GD_TUNE_KINDS        5
int gd_tune_reset(gd_handle* h);                         /* forget every measured choice */
/* Pin kind's choice for every size (variant >= 0), or return it to measuring (-1). */
int gd_tune_set(gd_handle* h, int kind, int variant);
/* The choice a launch of kind over n messages (sub: the bucketing's messages-a-range class, else 0)
 * would take: the pinned or measured variant, or -1 while still measuring. */
int gd_tune_get(gd_handle* h, int kind, uint64_t n, uint32_t sub, int* variant);
/* Collective over the handle's communicator (gd_comm_init*): every rank contributes its finished
 * measurements (best time per message of each variant of each kind and size class) and every rank
 * keeps, per entry any rank finished, the variant with the least summed time -- the same pick on every
 * rank.  Entries no rank finished keep measuring. */
int gd_tune_agree(gd_handle* h);

/* The handle's communicator: its rank count and this handle's rank as the transport reports them
 * (RCCL: ncclCommCount / ncclCommUserRank), and the transport. */
#define GD_COMM_NONE  0
#define GD_COMM_RCCL  1   /* gd_comm_init */
#define GD_COMM_LOCAL 2   /* gd_comm_init_local (in-process device copies) */
int gd_comm_info(gd_handle* h, int* n_ranks, int* rank, int* transport);

/* ---- probe indexes (round 6) -------------------------------------------------------------------
 * The compact probe indexes mirror the directory table slot for slot.  AddSingleActivation /
 * AddActivation / RemoveActivation batches (gd_dir_register*, gd_dir_upsert, gd_dir_unregister) keep
 * them current by re-projecting the slots they touched -- the reference's O(1) dictionary updates
 * (GrainDirectoryPartition.cs:304-363) stay O(batch); other directory changes (rehash, clear, silo
 * removal, merge, split, handoff) leave them to a full rebuild (two streaming passes) at the next large
 * route.  Keys an index does not hold (N0 != 0, a grain class or N1 it does not cover) are probed in
 * the directory per message.  Read-only statistics: */
typedef struct gd_index_stats {
    uint64_t builds;          /* full builds since gd_create                                      */
    uint64_t synced_slots;    /* table slots re-projected by directory batches                    */
    double   last_build_ms;   /* host wall time of the last build (both passes, one read-back)    */
    uint32_t current;         /* 1: the indexes match the table now                               */
    uint32_t types8;          /* grain classes (TypeCodeData) the 8-B index holds                 */
    uint32_t act_bits8;       /* its activation and silo field widths                             */
    uint32_t silo_bits8;
    uint32_t n0_live;         /* at the last build: live entries with N0 != 0 (directory probe)    */
    uint32_t out8;            /* live entries projected since the build that the 8-B index does not
                                 hold or redirects to the directory (incl. the build's own)         */
} gd_index_stats;
int gd_index_stats_get(gd_handle* h, gd_index_stats* out);
/* Diagnostic (no reference counterpart; bench.py's roofline.route_bound): gd_route_device's memory
 * bound over the current 8-B index -- the route kernel's launch shape, key reads, one 64-B index group
 * read per message at the key's home and its silo / act / status writes, without the ring search,
 * the walk past the home group or the directory fallback.  The outputs are NOT route results.
 * GD_EINVAL when the directory has no 8-B index. */
int gd_route_bound_device(gd_handle* h, const gd_key* d_keys, uint32_t n, uint32_t* d_silo, uint32_t* d_act,
                          uint8_t* d_status);

/* ---- frame encoder: Message.SetTargetPlacement + Message.Serialize for a batch -------
 * The counterpart of gd_decode_frames: the frames of a routed batch leave with their address written.
 * Per message the reference does two things after AddressMessage found the activation:
 *   Message.SetTargetPlacement (Message.cs:629-639, from Dispatcher.cs:753-767) sets TargetActivation,
 *     TargetSilo, IsNewPlacement (only ever to true) and NewGrainType (unless String.IsNullOrEmpty);
 *   Message.Serialize (Message.cs:481-516, HeadersContainer.Serializer :1126-1245) re-emits
 *     [int32 headerLength][int32 bodyLength][headers][body].
 * Here, for input frame i with route outputs silo[i], act[i], status[i]:
 *   TargetActivation = the ActivationId of act[i] (gd_activation_ids_set) as a UniqueKey: N0, N1,
 *     TypeCodeData, null KeyExt (int32 -1): 28 B (BinaryTokenStreamWriter.cs:37-49), after SendingSilo and
 *     before TargetGrain; a TargetActivation already there is replaced, its KeyExt string included.
 *   TargetSilo = silos[silo[i]] as ip[16], port, generation: 24 B (BinaryTokenStreamWriter.cs:485-513), after
 *     TargetGrain -- after TargetObserver when that is present, i.e. at the end of the header -- and before
 *     TransactionInfo; replaced if present.
 *   IsNewPlacement, when placed[i] == GD_PLACED_NEW: the True token (byte 3) after AlwaysInterleave and
 *     before ReadOnly; a token already there becomes True.  Any other placed[i] (or placed NULL) leaves the
 *     frame's own field as it is.
 *   NewGrainType, when new_type[i] indexes a non-empty string of the configured table: int32 UTF-8 length +
 *     bytes after IsUnordered and before RejectionInfo; replaced if present.  0xFFFFFFFF, an index >= n_types,
 *     an empty string or new_type NULL leave the frame's own field as it is.
 *   The mask gains the bits of the written fields, headerLength is rewritten, bodyLength is not; every other
 *   byte of the header, and the body, is copied in order.
 * Encode status, one byte per input frame, decided in this order:
 *   route status other than GD_ROUTE_OK / GD_ROUTE_ADDRESSED  -> GD_ENC_SKIPPED (a miss has no address; system
 *     targets need ActivationId.GetSystemActivation, Dispatcher.cs:785-800: both stay in C#)
 *   the decoder's GD_FRAME_MALFORMED length conditions          -> GD_ENC_MALFORMED
 *   GD_ROUTE_ADDRESSED (complete address, Dispatcher.cs:718)    -> GD_ENC_COPIED, a byte-for-byte copy
 *   CacheInvalidationHeader or RequestContext present, or TargetObserver and TransactionInfo both present (an
 *     insertion point lies behind an object-serialized field)   -> GD_ENC_FALLBACK, C# serializes it.  With
 *     GD_OPT_WALK_INVALIDATION 1 a CacheInvalidationHeader alone does not: the field is stepped over (a
 *     negative count or entries past the header: GD_ENC_MALFORMED) and copied through in front of Category
 *   the header walk runs off the header                          -> GD_ENC_MALFORMED
 *   silo[i] >= n_silos                                           -> GD_ENC_NO_SILO
 *   act[i] has no ActivationId (index past the map, or all zero) -> GD_ENC_NO_ID
 *   else                                                         -> GD_ENC_OK, the patched frame
 * Only OK and COPIED frames contribute bytes.  Output frame j is input frame order[j] (order: a permutation
 * of 0..n-1, e.g. gd_send_queues' perm; NULL = batch order): out_off[j] is its first byte in out_buf,
 * out_off[n] the total, so sender queue q of gd_send_queues owns the bytes
 * [out_off[offsets[q]], out_off[offsets[q + 1]]) -- one socket write.
 * Capacity: the total is compared with out_cap on the device.  If it is larger, nothing is written to
 * out_buf, out_off is still complete (out_off[n] = the size needed) and the handle's device error word is
 * raised: gd_encode_frames returns GD_EFULL, gd_encode_frames_device reports it at the next checked
 * synchronisation (as the asynchronous directory batches do).  Frames must be disjoint ranges of buf.
 * Totals are 32-bit: a call whose bound buf_len + n * (57 + longest configured type string) reaches 2^32 is
 * refused with GD_EINVAL (no 64-bit scan).  n == 0 is valid and writes out_off[0] = 0.
 * gd_encode_configure may be repeated; it synchronises the handle first.  type_off[0] = 0, n_types + 1
 * non-decreasing entries; a type string holds at most 65520 bytes.  The batch calls return GD_ESTATE before
 * it, and inside a hipGraph capture. */
#define GD_ENC_OK        0
#define GD_ENC_COPIED    1
#define GD_ENC_SKIPPED   2
#define GD_ENC_FALLBACK  3
#define GD_ENC_MALFORMED 4
#define GD_ENC_NO_ID     5
#define GD_ENC_NO_SILO   6
#define GD_ENC_NO_TYPE   0xFFFFFFFFu
int gd_encode_configure(gd_handle* h, const gd_silo_addr* silos, uint32_t n_silos, const uint8_t* type_utf8,
                        const uint32_t* type_off, uint32_t n_types);
/* Device pointers, enqueue only, no host read-back.  d_placed, d_new_type, d_order may be NULL. */
int gd_encode_frames_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                            uint32_t n, const uint32_t* d_silo, const uint32_t* d_act, const uint8_t* d_status,
                            const uint8_t* d_placed, const uint32_t* d_new_type, const uint32_t* d_order,
                            uint8_t* d_out_buf, uint64_t out_cap, uint64_t* d_out_off, uint8_t* d_enc_status);
/* Host pointers, synchronous; *out_total (may be NULL) = out_off[n]. */
int gd_encode_frames(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                     const uint32_t* silo, const uint32_t* act, const uint8_t* status, const uint8_t* placed,
                     const uint32_t* new_type, const uint32_t* order, uint8_t* out_buf, uint64_t out_cap,
                     uint64_t* out_off, uint8_t* enc_status, uint64_t* out_total);

/* ---- response writer: CreateResponseMessage / CreateRejectionResponse + Serialize for a batch ----
 * The answer to a request is built by MessageFactory.CreateResponseMessage (MessageFactory.cs:49-100, from
 * Dispatcher.SendResponse, Dispatcher.cs:769-783) or CreateRejectionResponse (:102-111, from
 * Dispatcher.RejectMessage :203-222, IncomingMessageAgent.cs:104, MessageCenter.SendRejection :193-197) and then
 * serialized (Message.cs:481-516).  Here the request frames are read where the receive stages left them and the
 * answers are written as frames, output frame j answering input frame order[j].
 *   kind[i]: GD_RSP_NONE (no answer), GD_RSP_RESPONSE (result[i]: 0 Success, 1 Error) or GD_RSP_REJECTION
 *   (rejection_type[i]: Message.RejectionTypes, 0 Transient, 1 Overloaded, 3 Unrecoverable ...; info[i]: an index
 *   into gd_respond_configure's strings, GD_RSP_NO_INFO or any index >= n_info: none).  Any other kind is NONE.
 * For a request with mask m the answer's header is written in HeadersContainer.Serializer order (Message.cs:
 * 1126-1244) with the mask GetHeadersMask (:1075-1117) gives for the message CreateResponseMessage builds:
 *   Category         copied when the request has it and the byte is not 0 (the enum default)
 *   DebugContext     copied when present with length > 0 (String.IsNullOrEmpty)
 *   Direction        always, byte 1 (Response)
 *   TimeToLive, CorrelationId   copied when present
 *   AlwaysInterleave, ReadOnly  bit set and a True token (3) written only when the request's token is 3; a request
 *                    carrying the bit with any other token loses it
 *   RejectionInfo    kind REJECTION and info[i] names a non-empty string: int32 length + bytes
 *   RejectionType    kind REJECTION and type != 0: one byte (Transient is the enum default: absent)
 *   Result           byte 2 for a rejection, byte 1 for result[i] == 1, absent for Success
 *   SendingActivation / SendingGrain / SendingSilo = the request's TargetActivation / TargetGrain / TargetSilo,
 *                    each with its KeyExt string bytes as they stand; SendingActivation only when TargetGrain is
 *                    present
 *   TargetActivation / TargetGrain / TargetSilo = the request's SendingActivation / SendingGrain / SendingSilo;
 *                    TargetActivation only when SendingGrain is present
 *   TransactionInfo  the request's bytes from the end of its last sized field to the end of the header, when the
 *                    bit is set
 *   dropped          ForwardCount, ResendCount, GenericGrainType, NewGrainType, IsNewPlacement, IsUnordered,
 *                    TargetObserver, the request's own RejectionInfo / RejectionType / Result and RequestContext,
 *                    the mask-only bits 25, 26 and 28, and bytes behind the last field of a header without
 *                    TransactionInfo
 * headerLength is recomputed; bodyLength is the supplied body's length: the body of answer i is
 * body[body_off[i] .. body_off[i + 1]) (body_off: n + 1 non-decreasing entries), copied as given -- the library
 * invents no body bytes, the caller serializes the Response object or the null exception.
 * RequestContextExtensions.Export is the responding thread's ambient context: a caller with a non-empty one keeps
 * C# for that message (kind NONE).
 * Status, one byte per input frame, decided in this order:
 *   kind NONE                                                    -> GD_RSPST_SKIPPED
 *   the decoder's GD_FRAME_MALFORMED length conditions           -> GD_RSPST_MALFORMED
 *   CacheInvalidationHeader present (object-serialized ahead of Direction, which cannot then be read)
 *                                                                -> GD_RSPST_FALLBACK
 *     With GD_OPT_WALK_INVALIDATION 1 the field is stepped over instead (a negative count or entries past the
 *     header: the next line's GD_RSPST_MALFORMED).  CreateResponseMessage copies the header
 *     (MessageFactory.cs:90): with count > 0 the answer carries the request's count and entries, byte for byte,
 *     in front of Category; with count 0 the answer's mask drops the bit (the Deserializer builds no list then,
 *     Message.cs:1254-1265).  One such frame stays GD_RSPST_FALLBACK, decided last, where it would have been
 *     GD_RSPST_OK: count > 0, a Category byte present with the enum's default value (the answer drops it) and a
 *     non-empty DebugContext behind it (kept) -- the entries and DebugContext would be two runs of the request,
 *     and the plan record has no run left.  The reference's serializer never writes a default-valued Category
 *   the walk to Direction runs off the header                    -> GD_RSPST_MALFORMED
 *   the request's Direction byte present and != 0 (RejectMessage :209-221; a frame without Direction counts as a
 *     request)                                                   -> GD_RSPST_DISCARDED
 *   RequestContext present, or TargetObserver and TransactionInfo both present
 *                                                                -> GD_RSPST_FALLBACK
 *   the walk through TargetGrain runs off the header             -> GD_RSPST_MALFORMED
 *   TargetGrain a system target (UniqueKey category 1) without TargetActivation: the answer needs
 *     ActivationId.GetSystemActivation (MessageFactory.cs:79-82) -> GD_RSPST_FALLBACK
 *   the rest of the walk runs off the header                     -> GD_RSPST_MALFORMED
 *   else                                                         -> GD_RSPST_OK
 * Only OK frames contribute bytes.  order, out_off[n + 1], out_cap, GD_EFULL (nothing written, out_off still
 * complete, the handle's device error word) and n == 0 are gd_encode_frames*'s.  Totals are 32-bit: a call whose
 * bound buf_len + body bytes + n * (16 + longest info string) reaches 2^32 is refused with GD_EINVAL; the device
 * form cannot see the body bytes, checks the rest and leaves body_off[n] to the caller.  d_result,
 * d_rejection_type, d_info, d_body / d_body_off (a pair) and d_order may each be NULL: Success, Transient, no
 * info, empty bodies, batch order.  Frames must be disjoint ranges of buf.
 * gd_respond_configure installs the RejectionInfo strings (the reference's hold Message.ToString() and exception
 * text and cannot be reproduced: the caller picks one by index, as for NewGrainType).  It may be repeated (n_info
 * may be 0) and synchronises the handle first; info_off[0] = 0, n_info + 1 non-decreasing entries.
 * gd_respond_frames* returns GD_ESTATE before it, and inside a hipGraph capture.
 * gd_respond_kinds*: kind / rejection type from the turn and receive statuses: GD_TURN_REJECT_OVERLOADED ->
 * REJECTION, Overloaded (1); GD_TURN_REJECT_TRANSIENT -> REJECTION, Transient (0); else, with recv_status given,
 * GD_RECV_REJECT_UNKNOWN -> REJECTION, Unrecoverable (3); GD_RECV_REJECT_OVERLOADED -> REJECTION, Overloaded (1);
 * anything else NONE (type 0).  recv_status may be NULL.
 * gd_silo_index*: wire24 holds n 24-byte wire SiloAddresses (ip[16], port, generation; 4-byte aligned, e.g.
 * gd_frame_fields.sending_silo); silo[i] = the lowest index of that address in gd_encode_configure's table,
 * GD_NO_SILO when it is not there.  GD_ESTATE before gd_encode_configure.  Its output feeds gd_send_queues*,
 * whose perm is then `order` here: each sender queue's answers are one contiguous byte run. */
#define GD_RSP_NONE      0
#define GD_RSP_RESPONSE  1
#define GD_RSP_REJECTION 2
#define GD_RSPST_OK        0
#define GD_RSPST_SKIPPED   1
#define GD_RSPST_MALFORMED 2
#define GD_RSPST_DISCARDED 3
#define GD_RSPST_FALLBACK  4
#define GD_RSP_NO_INFO 0xFFFFFFFFu
int gd_respond_configure(gd_handle* h, const uint8_t* info_utf8, const uint32_t* info_off, uint32_t n_info);
/* Device pointers, enqueue only. */
int gd_respond_kinds_device(gd_handle* h, const uint8_t* d_turn, const uint8_t* d_recv_status, uint32_t n,
                            uint8_t* d_kind, uint8_t* d_rejection_type);
int gd_silo_index_device(gd_handle* h, const uint8_t* d_wire24, uint32_t n, uint32_t* d_silo);
int gd_respond_frames_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                             uint32_t n, const uint8_t* d_kind, const uint8_t* d_result,
                             const uint8_t* d_rejection_type, const uint32_t* d_info, const uint8_t* d_body,
                             const uint64_t* d_body_off, const uint32_t* d_order, uint8_t* d_out_buf, uint64_t out_cap,
                             uint64_t* d_out_off, uint8_t* d_rsp_status);
/* Host pointers, synchronous; *out_total (may be NULL) = out_off[n]. */
int gd_respond_kinds(gd_handle* h, const uint8_t* turn, const uint8_t* recv_status, uint32_t n, uint8_t* kind,
                     uint8_t* rejection_type);
int gd_silo_index(gd_handle* h, const uint8_t* wire24, uint32_t n, uint32_t* silo);
int gd_respond_frames(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                      const uint8_t* kind, const uint8_t* result, const uint8_t* rejection_type, const uint32_t* info,
                      const uint8_t* body, const uint64_t* body_off, const uint32_t* order, uint8_t* out_buf,
                      uint64_t out_cap, uint64_t* out_off, uint8_t* rsp_status, uint64_t* out_total);

/* ---- request writer: CreateMessage + SendRequest + SetTargetPlacement + Serialize for a batch ----
 * A grain call becomes a message in MessageFactory.CreateMessage (MessageFactory.cs:21-47, from InsideRuntimeClient.
 * SendRequest, InsideRuntimeClient.cs:120-229); SendRequestMessage fills in the sender, the target, DebugContext,
 * GenericGrainType and TimeToLive; Dispatcher.SendMessage addresses it (gd_route), calls SetTargetPlacement
 * (Message.cs:629-639) and the message is serialized (Message.cs:481-516).  Here the frame
 * [int32 headerLength][int32 bodyLength][header][body] is written from a few words per message: no C# Message,
 * no HeadersContainer, no source frame.  For message i the header is what HeadersContainer.Serializer
 * (Message.cs:1126-1245) writes under the mask GetHeadersMask (:1075-1117) gives, in this order:
 *   Category          always, byte 2 (Categories.Application)
 *   DebugContext      when debug[i] indexes a non-empty string of gd_request_configure: int32 UTF-8 length + bytes
 *   Direction         always: byte 0 (Request), byte 2 (OneWay) with GD_REQ_ONE_WAY
 *   TimeToLive        ttl_ticks, 8 bytes as given (the reference writes ResponseTimeout minus the time since
 *                     creation: the value is the caller's), unless ttl_ticks == GD_TTL_NONE, the message is OneWay,
 *                     or GD_REQ_NO_TTL is set (system grains: Message.IsExpirableMessage, Message.cs:304-313)
 *   GenericGrainType  when generic[i] indexes a non-empty string of the same table
 *   CorrelationId     always, id_base + i, 8 bytes (CorrelationId.GetNext for a batch: the caller reserves n ids)
 *   AlwaysInterleave, IsNewPlacement, ReadOnly, IsUnordered   the mask bit and a True token (byte 3) each:
 *                     GD_REQ_ALWAYS_INTERLEAVE / _READ_ONLY / _UNORDERED; IsNewPlacement when addressed and
 *                     placed[i] == GD_PLACED_NEW (the encoder's rule); absent otherwise
 *   NewGrainType      when addressed and new_type[i] indexes a non-empty string of gd_encode_configure's type table
 *   SendingActivation the ActivationId of sender_act[i] (gd_activation_ids_set) as a UniqueKey, null KeyExt: 28 B
 *   SendingGrain      sender_grain[i], its KeyExt from sender_ext when given (else null)
 *   SendingSilo       gd_encode_configure's silos[gd_config.my_silo]: 24 B
 *   TargetActivation  when addressed: the ActivationId of act[i], as gd_encode_frames writes it
 *   TargetGrain       target[i], its KeyExt from target_ext when given
 *   TargetSilo        when addressed: silos[silo[i]], as gd_encode_frames writes it
 *   mask-only bits    26 (IsUsingInterfaceVersion) with GD_REQ_IFACE_VERSION, 28 (IsTransactionRequired) with
 *                     GD_REQ_TXN_REQUIRED
 *   never written     ForwardCount, ResendCount, Result, RejectionType / Info, CacheInvalidationHeader,
 *                     RequestContext, TargetObserver, TransactionInfo
 * "Addressed": the route arrays (d_silo, d_act, d_status: together or not at all) are given and
 * status[i] == GD_ROUTE_OK.  The body is body[body_off[i] .. body_off[i + 1]), copied as given (gd_respond_frames'
 * conventions: n + 1 non-decreasing entries, body and body_off a pair, the library invents no body bytes).
 * A KeyExt is gd_key_ext's: length[i] = GD_KEYEXT_NULL, or the UTF-8 bytes at offset[i]; the struct is a host
 * struct, its arrays device pointers in the device forms.
 * Status, one byte per message, decided in this order:
 *   a target_ext / sender_ext length of GD_KEYEXT_HOST (or any other length below -1, or a string that runs
 *     past bytes_len)                                                -> GD_REQ_FALLBACK
 *   TargetGrain a system target (UniqueKey category 1: ActivationId.GetSystemActivation and the Ping / System
 *     categories, InsideRuntimeClient.cs:182-189)                     -> GD_REQ_FALLBACK
 *   sender_act[i] has no ActivationId (past the map, or all zero)     -> GD_REQ_NO_ID
 *   addressed and silo[i] >= n_silos                                  -> GD_REQ_NO_SILO
 *   addressed and act[i] has no ActivationId                          -> GD_REQ_NO_ID
 *   addressed                                                         -> GD_REQ_OK
 *   else (a miss, any other route status, no route arrays)            -> GD_REQ_UNADDRESSED: the frame is written
 *     without TargetActivation, TargetSilo, IsNewPlacement and NewGrainType; C# takes it to AddressMessageAsync
 * Only OK and UNADDRESSED frames contribute bytes.  order, out_off[n + 1], out_cap and GD_EFULL (nothing written,
 * out_off still complete, the handle's device error word) and n == 0 are gd_encode_frames*'s.  Totals are 32-bit:
 * a call whose bound n * (206 + 2 * longest request string + longest type string) + KeyExt bytes + body bytes
 * reaches 2^32 is refused with GD_EINVAL; the device forms cannot see the KeyExt lengths and body_off, check the
 * rest and leave those bytes to the caller.  GD_ESTATE before gd_encode_configure or gd_request_configure, when
 * gd_config.my_silo is not in gd_encode_configure's table, and inside a hipGraph capture.
 * target_ext, sender_ext, options, generic, debug, body / body_off may be NULL: no KeyExt, options 0, no strings,
 * empty bodies.  Every route array and d_order may be NULL.
 * gd_request_configure installs the one string table debug[i] and generic[i] index (a string holds at most 65520
 * bytes; str_off[0] = 0, n_str + 1 non-decreasing entries; an index >= n_str names none).  It may be repeated
 * (n_str may be 0) and synchronises the handle first.
 * gd_request_send*: the head of the send path in one call, no host round trip in the device form: gd_route on
 * `target`, gd_send_queues with category Application and per message the TimeToLive its frame carries (ttl_ticks,
 * or none), then the writer with order = the send stage's perm, so each sender queue's requests are one contiguous
 * byte run: queue q owns [out_off[offsets[q]], out_off[offsets[q + 1]]).  It returns the outputs of all three
 * stages (d_queue may be NULL); GD_ESTATE before gd_send_configure too.  Frames of messages the send stage does
 * not queue (held, expired) are still written, in the trailing bucket.
 * Left to C#: observer references (TargetObserver), calls under a non-empty ambient RequestContext or an ambient
 * transaction (TransactionInfo.Fork), system-target senders and targets, body serialization, and the callback
 * object.  Registering the callbacks needs no device result: the ids are id_base + i and the caller knows which
 * calls are one-way, so it calls gd_callbacks_add* with its own arrays. */
#define GD_REQ_ONE_WAY           1u
#define GD_REQ_NO_TTL            2u
#define GD_REQ_ALWAYS_INTERLEAVE 4u
#define GD_REQ_READ_ONLY         8u
#define GD_REQ_UNORDERED         16u
#define GD_REQ_IFACE_VERSION     32u
#define GD_REQ_TXN_REQUIRED      64u
#define GD_REQ_OK          0
#define GD_REQ_UNADDRESSED 1
#define GD_REQ_FALLBACK    2
#define GD_REQ_NO_ID       3
#define GD_REQ_NO_SILO     4
#define GD_REQ_NO_STRING 0xFFFFFFFFu
typedef struct gd_request_batch {
    const gd_key*     target;        /* [n] TargetGrain                                         */
    const gd_key_ext* target_ext;    /* its KeyExt strings; NULL: every KeyExt null             */
    const gd_key*     sender_grain;  /* [n] SendingGrain                                        */
    const gd_key_ext* sender_ext;    /* NULL: every KeyExt null                                 */
    const uint32_t*   sender_act;    /* [n] the sender's activation index                       */
    const uint8_t*    options;       /* [n] GD_REQ_* bits; NULL: 0                              */
    const uint32_t*   generic;       /* [n] GenericGrainType string index; NULL: none           */
    const uint32_t*   debug;         /* [n] DebugContext string index; NULL: none               */
    int64_t           id_base;       /* CorrelationId of message 0                              */
    int64_t           ttl_ticks;     /* TimeToLive in TimeSpan ticks; GD_TTL_NONE: none         */
    const uint8_t*    body;          /* the bodies, concatenated; NULL (or body_off NULL): empty */
    const uint64_t*   body_off;      /* [n + 1]                                                 */
} gd_request_batch;
int gd_request_configure(gd_handle* h, const uint8_t* str_utf8, const uint32_t* str_off, uint32_t n_str);
/* Device pointers (the batch struct and the gd_key_ext structs are host structs), enqueue only, no host read-back. */
int gd_request_frames_device(gd_handle* h, const gd_request_batch* batch, uint32_t n, const uint32_t* d_silo,
                             const uint32_t* d_act, const uint8_t* d_status, const uint8_t* d_placed,
                             const uint32_t* d_new_type, const uint32_t* d_order, uint8_t* d_out_buf, uint64_t out_cap,
                             uint64_t* d_out_off, uint8_t* d_req_status);
int gd_request_send_device(gd_handle* h, const gd_request_batch* batch, uint32_t n, uint32_t* d_silo, uint32_t* d_act,
                           uint8_t* d_status, uint8_t* d_send_status, uint32_t* d_queue, uint32_t* d_perm,
                           uint32_t* d_offsets, uint8_t* d_out_buf, uint64_t out_cap, uint64_t* d_out_off,
                           uint8_t* d_req_status);
/* Host pointers, synchronous; *out_total (may be NULL) = out_off[n]. */
int gd_request_frames(gd_handle* h, const gd_request_batch* batch, uint32_t n, const uint32_t* silo,
                      const uint32_t* act, const uint8_t* status, const uint8_t* placed, const uint32_t* new_type,
                      const uint32_t* order, uint8_t* out_buf, uint64_t out_cap, uint64_t* out_off,
                      uint8_t* req_status, uint64_t* out_total);
int gd_request_send(gd_handle* h, const gd_request_batch* batch, uint32_t n, uint32_t* out_silo, uint32_t* out_act,
                    uint8_t* out_status, uint8_t* out_send_status, uint32_t* out_queue, uint32_t* out_perm,
                    uint32_t* out_offsets, uint8_t* out_buf, uint64_t out_cap, uint64_t* out_off, uint8_t* req_status,
                    uint64_t* out_total);

/* ---- forward writer: TryForwardRequest + AddressMessage + Serialize for a batch --------------------
 * A request that reached an invalid or stuck activation (gd_turns*: GD_TURN_FORWARD, GD_TURN_STUCK), or that stood
 * on the waiting list of a deactivated one (Dispatcher.ProcessRequestsToInvalidActivation, Dispatcher.cs:486-524),
 * is forwarded: Dispatcher.TryForwardRequest (:526-570) appends the old address to the CacheInvalidationHeader,
 * TryForwardMessage (:591-599) tests MayForward and counts ForwardCount up, ResendMessageImpl (:601-623) sets the
 * forwarding address or clears the target address and sends the message through AddressMessage again, and the
 * message is serialized (Message.cs:481-516).  Here the source frames are read where the receive stages left them
 * (buf, buf_len, frame_off[n], as gd_respond_frames) and the forwarded frames are written as frames, output frame
 * j being input frame order[j].
 *   kind[i]: GD_FWD_FORWARD, or GD_FWD_NONE (any other byte) for a message that does not leave here -- also the
 *     cross-cluster return of TryForwardRequest (:539-546), which stays in C#.
 *   old_act[i]: the invalid activation's index (its ActivationId: gd_activation_ids_set); GD_NO_ACTIVATION:
 *     oldAddress == null.  old_act NULL: none has one.
 *   fwd_silo[i], fwd_act[i]: the forwarding address; fwd_silo[i] == GD_NO_SILO: none.  The pair may be NULL.
 *   silo[i], act[i], status[i], placed[i], new_type[i]: the route's results for the frames that leave without a
 *     forwarding address, with gd_encode_frames' meaning; the three route arrays go together and, like placed and
 *     new_type, may be NULL.
 *   max_forward_count: SiloMessagingOptions.MaxForwardCount (default 2).  local_silo: this silo's index in
 *     gd_encode_configure's table (oldAddress is always an address on this silo).
 * The CacheInvalidationHeader is a sized field: HeadersContainer.Serializer writes an int32 count and then every
 * entry through the registered ActivationAddress serializer, which writes, with no type token, the SiloAddress
 * (24 B), the GrainId UniqueKey (24 B + KeyExt string) and the ActivationId UniqueKey (24 B + KeyExt string)
 * (Message.cs:1132-1140, :1363-1367; BuiltInTypes.cs:2059-2063; BinaryTokenStreamWriter.cs:27-35): 80 B an entry
 * for a long-keyed grain.  It stands first, right behind the mask.
 * The output header, in HeadersContainer.Serializer order (Message.cs:1126-1244):
 *   CacheInvalidationHeader  when old_act[i] names an activation: count = old count + 1 (1 when the field was
 *                     absent), the old entries as they stand, then one entry: silos[local_silo] (24 B), the
 *                     frame's own TargetGrain UniqueKey with its KeyExt bytes as they stand, the ActivationId of
 *                     old_act[i] with a null KeyExt (28 B); the mask gains bit 1.  Else as in the source.
 *                     (Message.AddToCacheInvalidationHeader, Message.cs:333-343; ahead of MayForward, as in C#.)
 *   ForwardCount      old value + 1 (absent counts as 0) as an int32, behind TimeToLive and in front of
 *                     GenericGrainType: replaced, or inserted; field and bit are dropped when the new value is 0
 *                     (GetHeadersMask, Message.cs:1093)
 *   forwarding address given: TargetActivation = the ActivationId of fwd_act[i] (28 B), TargetSilo =
 *                     silos[fwd_silo[i]], replaced or inserted at gd_encode_frames' positions; IsNewPlacement is
 *                     removed, token and bit (:612-613).  TargetGrain stays the frame's.
 *   no forwarding address: TargetActivation and TargetSilo are removed (:618-620); then, when status[i] ==
 *                     GD_ROUTE_OK, Message.SetTargetPlacement exactly as gd_encode_frames applies it:
 *                     TargetActivation, TargetSilo, IsNewPlacement by placed[i], NewGrainType by new_type[i].
 *                     Otherwise the frame leaves unaddressed, for AddressMessageAsync.
 *   everything else   headerLength is rewritten, bodyLength is not; every other header byte, and the body, is
 *                     copied in order (the encoder's copy rule; it also defines the result for frames the
 *                     reference's serializer would not emit).  TargetHistory is not a wire field.
 * Status, one byte per input frame, decided in this order:
 *   kind not GD_FWD_FORWARD                                        -> GD_FWDST_SKIPPED
 *   the decoder's GD_FRAME_MALFORMED length conditions; a negative invalidation count; the walk runs off the
 *     header (the walk ends in front of RequestContext, and behind TargetGrain when TargetObserver and
 *     TransactionInfo are both present)                             -> GD_FWDST_MALFORMED
 *   RequestContext present; TargetObserver and TransactionInfo both present; TargetGrain absent; TargetGrain a
 *     system target (SendSystemTargetMessage, :606-609)             -> GD_FWDST_FALLBACK, C# forwards it
 *   ForwardCount >= max_forward_count (MayForward, :627-630)        -> GD_FWDST_REJECT: no bytes here; the
 *     reference's rejection carries the extended invalidation header (MessageFactory.cs:90), which
 *     gd_respond_frames does not write: gd_forward_reject_frames* (below) writes it from this same batch
 *   old_act[i] names an activation and local_silo >= n_silos        -> GD_FWDST_NO_SILO
 *   old_act[i] names an activation without an ActivationId          -> GD_FWDST_NO_ID
 *   the address written (the forwarding address, else the route's): its silo >= n_silos -> GD_FWDST_NO_SILO,
 *     its activation without an ActivationId                        -> GD_FWDST_NO_ID
 *   else                                   -> GD_FWDST_OK_ADDRESSED, or GD_FWDST_OK_UNADDRESSED (no address written)
 * Only the two OK statuses contribute bytes.  target[i] (may be NULL) = the frame's TargetGrain for every status
 * but SKIPPED, MALFORMED and FALLBACK (zeros there): the caller routes or places the unaddressed frames without a
 * second decode.  order, out_off[n + 1], out_cap, GD_EFULL (nothing written, out_off still complete, the handle's
 * device error word) and n == 0 are gd_encode_frames*'s.  Totals are 32-bit: a frame gains at most the count (4),
 * one entry (80 + its TargetGrain KeyExt bytes), ForwardCount (4) and the encoder's 57 + the longest type string,
 * and the KeyExt bytes of all frames lie in buf, so a call whose bound
 *   2 * buf_len + n * (145 + longest configured type string)
 * reaches 2^32 is refused with GD_EINVAL.  Frames must be disjoint ranges of buf.  GD_ESTATE before
 * gd_encode_configure, and inside a hipGraph capture.
 * gd_forward_kinds*: GD_TURN_FORWARD and GD_TURN_STUCK -> GD_FWD_FORWARD, everything else GD_FWD_NONE.
 * gd_forward_send*: the chain, no host round trip in the device form: the plan; gd_route on `target`; the merge
 * into silo / act / status (a frame that does not leave: GD_NO_SILO, GD_NO_ACTIVATION, GD_ROUTE_UNDECODED; a
 * forwarding address wins over the route: its silo, its activation, GD_ROUTE_OK; a TargetGrain with a KeyExt
 * string: GD_ROUTE_KEYEXT; else the route's result); gd_send_queues with each frame's own Category (absent: 0)
 * and TimeToLive; then the writer with order = the send stage's perm and the address of every GD_ROUTE_OK message,
 * so each sender queue's forwarded frames are one contiguous byte run: queue q owns
 * [out_off[offsets[q]], out_off[offsets[q + 1]]).  It returns the outputs of all three stages (d_queue may be
 * NULL; target is required); GD_ESTATE before gd_send_configure too.  Misses leave unaddressed: gd_route_place* on
 * the returned keys is the caller's next step.
 * Left to C#: the cross-cluster return, system targets and FALLBACK frames.  The rejections of messages that may
 * not forward are gd_forward_reject_frames*' (below).  InvalidateCacheEntry -- on the receiving side, and the sending side's own call for the old
 * address (Dispatcher.cs:478, :497) -- is the sniff stage's (gd_sniff_invalidate*, gd_cache_invalidate*, below). */
#define GD_FWD_NONE    0
#define GD_FWD_FORWARD 1
#define GD_FWDST_OK_ADDRESSED   0
#define GD_FWDST_OK_UNADDRESSED 1
#define GD_FWDST_SKIPPED        2
#define GD_FWDST_MALFORMED      3
#define GD_FWDST_FALLBACK       4
#define GD_FWDST_REJECT         5
#define GD_FWDST_NO_SILO        6
#define GD_FWDST_NO_ID          7
typedef struct gd_forward_batch {
    const uint8_t*  buf;                /* the receive buffer                                      */
    uint64_t        buf_len;
    const uint64_t* frame_off;          /* [n] first byte of every frame                           */
    const uint8_t*  kind;               /* [n] GD_FWD_*                                            */
    const uint32_t* old_act;            /* [n] or NULL                                             */
    const uint32_t* fwd_silo;           /* [n] or NULL (with fwd_act)                              */
    const uint32_t* fwd_act;            /* [n] or NULL                                             */
    int32_t         max_forward_count;  /* SiloMessagingOptions.MaxForwardCount                    */
    uint32_t        local_silo;         /* index into gd_encode_configure's table                  */
} gd_forward_batch;
/* Device pointers (the batch struct is a host struct), enqueue only, no host read-back. */
int gd_forward_kinds_device(gd_handle* h, const uint8_t* d_turn, uint32_t n, uint8_t* d_kind);
int gd_forward_frames_device(gd_handle* h, const gd_forward_batch* batch, uint32_t n, const uint32_t* d_silo,
                             const uint32_t* d_act, const uint8_t* d_status, const uint8_t* d_placed,
                             const uint32_t* d_new_type, const uint32_t* d_order, uint8_t* d_out_buf, uint64_t out_cap,
                             uint64_t* d_out_off, uint8_t* d_fwd_status, gd_key* d_target);
int gd_forward_send_device(gd_handle* h, const gd_forward_batch* batch, uint32_t n, uint32_t* d_silo, uint32_t* d_act,
                           uint8_t* d_status, uint8_t* d_send_status, uint32_t* d_queue, uint32_t* d_perm,
                           uint32_t* d_offsets, uint8_t* d_out_buf, uint64_t out_cap, uint64_t* d_out_off,
                           uint8_t* d_fwd_status, gd_key* d_target);
/* Host pointers, synchronous; *out_total (may be NULL) = out_off[n]. */
int gd_forward_kinds(gd_handle* h, const uint8_t* turn, uint32_t n, uint8_t* kind);
int gd_forward_frames(gd_handle* h, const gd_forward_batch* batch, uint32_t n, const uint32_t* silo,
                      const uint32_t* act, const uint8_t* status, const uint8_t* placed, const uint32_t* new_type,
                      const uint32_t* order, uint8_t* out_buf, uint64_t out_cap, uint64_t* out_off,
                      uint8_t* fwd_status, gd_key* target, uint64_t* out_total);
int gd_forward_send(gd_handle* h, const gd_forward_batch* batch, uint32_t n, uint32_t* out_silo, uint32_t* out_act,
                    uint8_t* out_status, uint8_t* out_send_status, uint32_t* out_queue, uint32_t* out_perm,
                    uint32_t* out_offsets, uint8_t* out_buf, uint64_t out_cap, uint64_t* out_off, uint8_t* fwd_status,
                    gd_key* target, uint64_t* out_total);

/* ---- forward rejections: TryForwardRequest's failure arm + RejectMessage + Serialize for a batch ---
 * A request that must be forwarded but has been forwarded MaxForwardCount times already is rejected:
 * Dispatcher.TryForwardRequest (Dispatcher.cs:526-570) appends the old address to the message's
 * CacheInvalidationHeader -- ahead of MayForward --, TryForwardMessage (:591-599, :627-630) returns false without
 * counting ForwardCount up, RejectMessage(message, Transient, exc, str) (:203-222) answers a Request with
 * MessageFactory.CreateRejectionResponse (MessageFactory.cs:49-111) and drops any other direction, and
 * CreateResponseMessage copies the request's CacheInvalidationHeader (:90): the rejection carries the old entries
 * plus the one just appended.  These are the frames gd_forward_frames* marks GD_FWDST_REJECT; this stage takes the
 * same source frames and the same gd_forward_batch and writes their answers, output frame j being input frame
 * order[j].
 *   batch->buf, buf_len, frame_off, kind, old_act, max_forward_count, local_silo: gd_forward_frames*' meaning.
 *     fwd_silo and fwd_act are ignored.
 *   info[i]: an index into gd_respond_configure's strings, as gd_respond_frames' info; GD_RSP_NO_INFO or any index
 *     >= n_info: no RejectionInfo.  (The reference's string holds Message.ToString(): the caller's choice.)
 *   body, body_off: gd_respond_frames' pair (n + 1 non-decreasing entries); the serialized exc, or null, is the
 *     caller's.
 * The invalidation field is always walked, as in the forward writer, whatever GD_OPT_WALK_INVALIDATION is set to.
 * The answer's header, in HeadersContainer.Serializer order (Message.cs:1126-1244):
 *   CacheInvalidationHeader  when old_act[i] names an activation: count = old count + 1 (1 when the field was
 *                     absent), the old entries as they stand, then one entry exactly as the forward writer writes
 *                     it: silos[local_silo] (24 B), the frame's TargetGrain UniqueKey with its KeyExt bytes as they
 *                     stand, the ActivationId of old_act[i] with a null KeyExt (28 B); the mask has bit 1.
 *                     When old_act[i] == GD_NO_ACTIVATION, or old_act is NULL: a request's field with count > 0 is
 *                     copied byte for byte, one with count 0 is dropped, bit included, an absent one stays absent.
 *   everything behind it     what gd_respond_frames* writes for kind GD_RSP_REJECTION with rejection type 0
 *                     (Transient): Category dropped when its byte is 0, DebugContext dropped when empty, Direction
 *                     1, TimeToLive, CorrelationId and the two True tokens carried over, RejectionInfo by info[i],
 *                     no RejectionType byte, Result 2, Target* and Sending* exchanged, TransactionInfo kept,
 *                     ForwardCount and the rest of that contract's "dropped" list dropped.  headerLength is
 *                     recomputed; bodyLength is the supplied body's length.
 * The stage has no fallback of its own: the frame gd_respond_frames* keeps GD_RSPST_FALLBACK under the walk option
 * (entries, a default-valued Category byte, a non-empty DebugContext) is GD_FWDREJ_OK here.
 * Status, one byte per input frame, decided in this order:
 *   kind not GD_FWD_FORWARD                                          -> GD_FWDREJ_SKIPPED
 *   the forward writer's GD_FWDST_MALFORMED conditions               -> GD_FWDREJ_MALFORMED
 *   the forward writer's GD_FWDST_FALLBACK conditions (RequestContext present; TargetObserver and TransactionInfo
 *     both present; TargetGrain absent; a system target: they cover every FALLBACK of gd_respond_frames)
 *                                                                    -> GD_FWDREJ_FALLBACK
 *   ForwardCount < max_forward_count (absent counts as 0)            -> GD_FWDREJ_MAY_FORWARD: the forward writer's
 *   the Direction byte present and != 0 (Dispatcher.cs:209-221)      -> GD_FWDREJ_DISCARDED
 *   old_act[i] names an activation and local_silo >= n_silos         -> GD_FWDREJ_NO_SILO
 *   old_act[i] names an activation without an ActivationId           -> GD_FWDREJ_NO_ID
 *   else                                                             -> GD_FWDREJ_OK
 * Only OK frames contribute bytes.  On any batch the frames marked DISCARDED, NO_SILO, NO_ID or OK are exactly the
 * frames gd_forward_frames* marks GD_FWDST_REJECT, and the SKIPPED, MALFORMED and FALLBACK sets are the forward
 * writer's.  order, out_off[n + 1], out_cap, GD_EFULL (nothing written, out_off still complete, the handle's
 * device error word) and n == 0 are gd_encode_frames*'s.  Totals are 32-bit: the copied bytes are at most buf_len,
 * and a frame gains at most the count (4), one entry (80 + its TargetGrain KeyExt bytes, which lie in buf: buf_len
 * bounds their sum), Direction (1), the RejectionInfo length (4), Result (1) and the info string: 90 + the string.
 * A call whose bound
 *   2 * buf_len + body bytes + n * (90 + longest info string)
 * reaches 2^32 is refused with GD_EINVAL; the device form cannot see the body bytes, checks the rest and leaves
 * body_off[n] to the caller.  d_info, d_body / d_body_off (a pair) and d_order may each be NULL: no info, empty
 * bodies, batch order.  Frames must be disjoint ranges of buf.  GD_ESTATE before gd_encode_configure or
 * gd_respond_configure, and inside a hipGraph capture.
 * The answers leave as gd_respond_frames*' do: gd_silo_index* on the decoder's sending_silo, gd_send_queues*, and
 * its perm as `order` here.  ProcessRequestsToInvalidActivation(rejectMessages: true) needs nothing of this: it
 * appends no entry and is gd_respond_frames* with kind GD_RSP_REJECTION under GD_OPT_WALK_INVALIDATION. */
#define GD_FWDREJ_OK          0
#define GD_FWDREJ_SKIPPED     1
#define GD_FWDREJ_MALFORMED   2
#define GD_FWDREJ_FALLBACK    3
#define GD_FWDREJ_MAY_FORWARD 4
#define GD_FWDREJ_DISCARDED   5
#define GD_FWDREJ_NO_SILO     6
#define GD_FWDREJ_NO_ID       7
/* Device pointers (the batch struct is a host struct), enqueue only, no host read-back. */
int gd_forward_reject_frames_device(gd_handle* h, const gd_forward_batch* batch, uint32_t n, const uint32_t* d_info,
                                    const uint8_t* d_body, const uint64_t* d_body_off, const uint32_t* d_order,
                                    uint8_t* d_out_buf, uint64_t out_cap, uint64_t* d_out_off, uint8_t* d_rej_status);
/* Host pointers, synchronous; *out_total (may be NULL) = out_off[n]. */
int gd_forward_reject_frames(gd_handle* h, const gd_forward_batch* batch, uint32_t n, const uint32_t* info,
                             const uint8_t* body, const uint64_t* body_off, const uint32_t* order, uint8_t* out_buf,
                             uint64_t out_cap, uint64_t* out_off, uint8_t* rej_status, uint64_t* out_total);

/* ---- sniff stage: SniffIncomingMessage + InvalidateCacheEntry for a batch --------------------------
 * InsideRuntimeClient.SniffIncomingMessage (InsideRuntimeClient.cs:253-263) runs for every incoming message ahead of
 * everything else: for each address of its CacheInvalidationHeader it calls LocalGrainDirectory.InvalidateCacheEntry
 * (LocalGrainDirectory.cs:965-986): DirectoryCache.LookUp, then RemoveActivations(... t.Item2.Equals(activationId))
 * (:1146-1164).  The stage does that for the frames of a received batch (buf, buf_len, frame_off[n], as
 * gd_decode_frames) on the non-owner cache (gd_cache_configure).  No other entry point changes: gd_decode_frames*,
 * gd_encode_frames* and gd_respond_frames* still answer FALLBACK for frames that carry the header.
 *
 * 1. gd_sniff_frames*: the entries.  The header is walked as the forward writer walks it: int32 count, then per entry
 *    SiloAddress (24 B), GrainId UniqueKey (24 B + KeyExt string), ActivationId UniqueKey (24 B + KeyExt string).
 *    Per frame i:
 *      count[i]    entries the frame contributes; 0 without the header, and for a malformed frame.
 *      ent_off[n + 1]  the exclusive prefix of count; ent_off[n] = m, the batch's entries.
 *      status[i]   GD_SNIFF_NONE       mask bit 1 clear (the frame's length conditions hold);
 *                  GD_SNIFF_OK         the header walked; a count of 0 is OK with no entries;
 *                  GD_SNIFF_MALFORMED  the decoder's length conditions fail, the count is negative, a string length
 *                                      is below -1, or an entry runs past the header.  No entries.
 *      flags[i]    bit 0 (GD_SNIFF_FLAG_RETURNED) = the message's IsReturnedFromRemoteCluster as the reference's
 *                  deserializer would leave it.  The reference gives that header no wire form: GetHeadersMask
 *                  (Message.cs:1075-1117) never sets mask bit 25, the serializer writes no byte for it and the
 *                  deserializer (:1247-1356) never reads it, so a received message's value is false and bit 0 is
 *                  always 0.  A frame whose mask has bit 25 set is not one the reference's serializer wrote: it gets
 *                  bit 1 (GD_SNIFF_FLAG_UNKNOWN), C# decides; no byte is guessed at.  0 for a malformed frame.
 *    Per entry e in [ent_off[i], ent_off[i + 1]), in header order -- batch order x header order is the reference's
 *    call order:
 *      ent_frame[e]    i.
 *      ent_silo[e]     the SiloAddress' 24 wire bytes as six dwords (gd_frame_fields' silo layout).
 *      ent_grain[e]    the GrainId's three words.
 *      ent_ext_off[e], ent_ext_len[e]  the GrainId's KeyExt string: its absolute offset into buf and its UTF-8 length,
 *                      GD_KEYEXT_NULL for null.  The strings are not copied: {buf, ent_ext_off, ent_ext_len, buf_len}
 *                      is a gd_key_ext of the entries.
 *      ent_act_id[e]   the ActivationId's three words; all zeros for an ActivationId that carries a non-null KeyExt
 *                      string (the map of gd_activation_ids_set holds null-KeyExt ids only, and by UniqueKey.Equals
 *                      such an id equals none of them).
 *    Any output but count, ent_off and status may be NULL.  ent_cap = the entries the entry arrays hold: if
 *    m > ent_cap no entry is written, ent_off is still complete, and the handle's device error word is raised -- the
 *    host form returns GD_EFULL, the device form reports it at the next checked synchronisation (gd_encode_frames'
 *    rule).  n == 0 is GD_OK (ent_off[0] = 0).  Frames must be disjoint ranges of buf; an entry holds at least 80 B,
 *    so m <= buf_len / 80, and a call with buf_len / 80 >= 2^32 is GD_EINVAL, as is n > 2^31.  GD_ESTATE inside a
 *    hipGraph capture.
 *
 * 2. gd_cache_invalidate*: InvalidateCacheEntry(keys[k], act_ids[k]) for k = 0 .. m - 1 in order on the cache
 *    (GD_ESTATE before gd_cache_configure).  ext (may be NULL) keys KeyExt grains by their string, as
 *    gd_cache_lookup_ext.  The device form takes d_m (may be NULL): the live count on the device; the launch is sized
 *    by m, the arrays' capacity, and entries at or past *d_m are not read, have no effect and get no out[k]; *d_m
 *    above m (the sniff stage's GD_EFULL) processes nothing.  out[k]:
 *      GD_INV_MISS     LookUp missed -- also a grain an earlier entry of this batch removed.  NumAccesses counted.
 *      GD_INV_REMOVED  hit; the cached activation's ActivationId (gd_activation_ids_set) equals act_ids[k]: the entry
 *                      is removed as gd_cache_remove removes (counters, tombstone).
 *      GD_INV_KEPT     hit; another activation, or the cached empty list (silo GD_NO_SILO): the entry stays.
 *      GD_INV_HOST     hit; the entry is GD_ACT_MULTI: its list is C#'s, the entry stays.
 *      GD_INV_NO_ID    hit; the cached activation has no ActivationId in the map: the entry stays.
 *    Every hit, the removing one included, is a LookUp hit (AdaptiveGrainDirectoryCache.cs:90-109): it takes the next
 *    LRU generation in batch order and one NumAccesses++ on its entry, and accesses / hits of gd_cache_stats advance
 *    as gd_cache_lookup advances them.  A key the device cannot match (GD_KEYEXT_HOST, a string range outside
 *    bytes_len) is GD_INV_MISS without an access counted in the device form and GD_EINVAL (nothing done) in the host
 *    form, as gd_cache_remove_ext treats it.  Not done here: invalidateDirectoryAlso -> registrar.InvalidateCache
 *    (:981-985, multi-cluster) stays in C#, fed by flags; the entry's SiloAddress is not compared, because the
 *    reference does not compare it.
 *
 * 3. gd_sniff_invalidate*: the chain, no host read-back in the device form: gd_sniff_frames, then
 *    gd_cache_invalidate on (ent_grain, {buf, ent_ext_off, ent_ext_len}, ent_act_id) with d_m = ent_off + n and the
 *    capacity ent_cap; inv[e] is entry e's GD_INV_*.  ent_grain, ent_ext_off, ent_ext_len, ent_act_id and inv are
 *    required here (ent_cap > 0).  m > ent_cap: GD_EFULL as above and the cache is unchanged. */
#define GD_SNIFF_NONE      0
#define GD_SNIFF_OK        1
#define GD_SNIFF_MALFORMED 2
#define GD_SNIFF_FLAG_RETURNED 1
#define GD_SNIFF_FLAG_UNKNOWN  2
#define GD_INV_MISS    0
#define GD_INV_REMOVED 1
#define GD_INV_KEPT    2
#define GD_INV_HOST    3
#define GD_INV_NO_ID   4
typedef struct gd_sniff_out {
    uint32_t* count;        /* [n]                                                     */
    uint32_t* ent_off;      /* [n + 1]                                                 */
    uint8_t*  status;       /* [n] GD_SNIFF_*                                          */
    uint8_t*  flags;        /* [n] GD_SNIFF_FLAG_*, or NULL                            */
    uint32_t* ent_frame;    /* [ent_cap] or NULL                                       */
    uint32_t* ent_silo;     /* [ent_cap * 6] or NULL                                   */
    gd_key*   ent_grain;    /* [ent_cap] or NULL                                       */
    uint64_t* ent_ext_off;  /* [ent_cap] or NULL                                       */
    int32_t*  ent_ext_len;  /* [ent_cap] or NULL                                       */
    gd_key*   ent_act_id;   /* [ent_cap] or NULL                                       */
} gd_sniff_out;
/* Device pointers (the out struct is a host struct of device pointers), enqueue only, no host read-back. */
int gd_sniff_frames_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                           uint32_t n, const gd_sniff_out* d_out, uint32_t ent_cap);
int gd_cache_invalidate_device(gd_handle* h, const gd_key* d_keys, const gd_key_ext* d_ext, const gd_key* d_act_ids,
                               uint32_t m, const uint32_t* d_m, uint8_t* d_out);
int gd_sniff_invalidate_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len, const uint64_t* d_frame_off,
                               uint32_t n, const gd_sniff_out* d_out, uint32_t ent_cap, uint8_t* d_inv);
/* Host pointers, synchronous; *out_m (may be NULL) = ent_off[n].  Only the first m entries are written. */
int gd_sniff_frames(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                    const gd_sniff_out* out, uint32_t ent_cap, uint32_t* out_m);
int gd_cache_invalidate(gd_handle* h, const gd_key* keys, const gd_key_ext* ext, const gd_key* act_ids, uint32_t m,
                        uint8_t* out);
int gd_sniff_invalidate(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off, uint32_t n,
                        const gd_sniff_out* out, uint32_t ent_cap, uint8_t* inv, uint32_t* out_m);

/* ---- batched Catalog.GetOrCreateActivation: activations for a received batch ------------
 * A message gd_receive* leaves GD_RECV_NULL_CONTEXT met no Valid activation.  Its closure
 * (Dispatcher.ReceiveMessage, Core/Dispatcher.cs:75-201) first tests IsExpired (:79-85), then runs
 * Catalog.GetOrCreateActivation (Catalog/Catalog.cs:443-518) under lock (activations): TryGetActivationData finds
 * the activation in whatever state; or a dummy ActivationData is created and recorded (RegisterMessageTarget ->
 * ActivationDirectory.RecordNewTarget, Catalog/ActivationDirectory.cs:86-93) when the message carries
 * IsNewPlacement; or NonExistentActivationException leads to ProcessRequestToInvalidActivation +
 * UnregisterAfterNonexistingActivation (requests) or InvalidateCacheEntry (responses).  gd_activate* is that step
 * for a batch in arrival order, on the activation directory of gd_actdir_*.  (The reference runs these closures on
 * the null context in no fixed order; arrival order is the batch model, as for every stage of this library.)
 *
 * Per message: ctx and recv_status as gd_receive* gave them; target_grain (not read: C# builds the ActivationData
 * from it through new_idx) and target_activation; direction (NULL = every message a Request, 0xFF = absent =
 * Request); ttl (NULL = none, GD_TTL_NONE = no value); new_placement (NULL = all 0; Message.IsNewPlacement, true
 * only for the value 1).  Scalars: terminating = SiloStatusOracle.CurrentStatus.IsTerminating() (nothing is
 * created); ctx_base and new_ctx[cap_new] (NULL: ctx_base + k), the contexts offered to new activations.
 *
 * Only messages with recv_status == GD_RECV_NULL_CONTEXT take part; every other message gets GD_ACTV_NONE and its
 * ctx / status are copied through.  Per participating message, one by one in array order:
 *   1. ttl has a value and is <= 0: GD_ACTV_EXPIRED; no state is touched.
 *   2. the ActivationId is in the directory as an activation entry, in any state -- there before the batch or
 *      created by an earlier message of it: GD_ACTV_FOUND, ctx_out = its context, status_out = GD_RECV_ACTIVATION.
 *      A stored context >= n_ctx: GD_ACTV_HOST and the call fails with GD_EINVAL, as gd_receive's.
 *   3. present only as a system-target entry: GD_ACTV_HOST (the reference keeps two dictionaries, the library one
 *      table; C# handles this corner).
 *   4. absent, new_placement set, not terminating: a candidate.  The k-th candidate of the batch (arrival order)
 *      proposes new_ctx[k], or ctx_base + k.  The first candidate of an ActivationId creates the entry {its
 *      proposal, flags 0}: not Valid, no system target, no stateless worker -- ActivationState.Create.  It gets
 *      GD_ACTV_CREATED, ctx_out = the proposal, status_out = GD_RECV_ACTIVATION.  Later candidates of the id fall
 *      under rule 2, so the proposals are sparse, as gd_route_place's.  *n_proposed = the candidates; new_idx
 *      lists the creating messages in arrival order (C# builds an ActivationData for each and runs
 *      SetupActivationInstance / InitActivation).
 *   5. otherwise GD_ACTV_NONEXISTENT (Request, OneWay) or GD_ACTV_NONEXISTENT_RESPONSE; ctx / status copied
 *      through.  gone_idx lists the GD_ACTV_NONEXISTENT messages in arrival order: the input of gd_forward_* and
 *      the UnregisterAfterNonexistingActivation list.
 * The batch is refused whole -- nothing is created, every participating message rules 1-3 do not decide gets
 * GD_ACTV_HOST, n_new = n_gone = 0 -- when *n_proposed > cap_new or one of the first cap_new proposals is >= n_ctx.
 * The host form then returns GD_EINVAL after writing the outputs; the device form's caller compares the
 * n_proposed word with cap_new (gd_callbacks_expire's convention), and a proposal out of range fails the next
 * synchronising call with GD_EINVAL, as gd_receive's context check.  new_ctx NULL and ctx_base + cap_new > n_ctx:
 * GD_EINVAL up front.
 *
 * Outputs: kind[n]; ctx_out[n] / status_out[n], which may be the inputs ctx / recv_status; new_idx[n] with the word
 * n_new and gone_idx[n] with n_gone, each both or neither; the word n_proposed.  The words are device words in
 * the device form and host words in the host form.  The device form only enqueues: room for min(n, cap_new) new
 * entries is reserved first, from a bound kept on the host, with one counter read-back (GD_ESTATE inside a
 * capture) only when the bound cannot tell; its claims run a fixed number of gated passes, and a batch they do not
 * settle fails the next synchronising call with GD_ETIMEOUT, as gd_callbacks_add_device's.  The host form is
 * synchronous, GD_ESTATE inside a capture.
 *
 * Left to C#: GetGrainTypeInfo, the NewGrainType / GenericGrainType strings, the ActivationData object and
 * InitActivation for new_idx, the later gd_actdir_set_flags(GD_ACTDIR_VALID), statistics and logging. */
#define GD_ACTV_NONE                 0
#define GD_ACTV_FOUND                1
#define GD_ACTV_CREATED              2
#define GD_ACTV_EXPIRED              3
#define GD_ACTV_HOST                 4
#define GD_ACTV_NONEXISTENT          5
#define GD_ACTV_NONEXISTENT_RESPONSE 6
int gd_activate_device(gd_handle* h, const uint32_t* d_ctx, const uint8_t* d_recv_status, const gd_key* d_target_grain,
                       const gd_key* d_target_activation, const uint8_t* d_direction, const int64_t* d_ttl,
                       const uint8_t* d_new_placement, uint32_t n, uint32_t n_ctx, int terminating, uint32_t ctx_base,
                       const uint32_t* d_new_ctx, uint32_t cap_new, uint8_t* d_kind, uint32_t* d_ctx_out,
                       uint8_t* d_status_out, uint32_t* d_new_idx, uint32_t* d_n_new, uint32_t* d_gone_idx,
                       uint32_t* d_n_gone, uint32_t* d_n_proposed);
int gd_activate(gd_handle* h, const uint32_t* ctx, const uint8_t* recv_status, const gd_key* target_grain,
                const gd_key* target_activation, const uint8_t* direction, const int64_t* ttl,
                const uint8_t* new_placement, uint32_t n, uint32_t n_ctx, int terminating, uint32_t ctx_base,
                const uint32_t* new_ctx, uint32_t cap_new, uint8_t* out_kind, uint32_t* out_ctx, uint8_t* out_status,
                uint32_t* out_new_idx, uint32_t* out_n_new, uint32_t* out_gone_idx, uint32_t* out_n_gone,
                uint32_t* out_n_proposed);
/* The chains: gd_receive_device -> gd_activate_device -> gd_turns_device on the resolved ctx / status (written in
 * place into d_ctx / d_status), no host round trip.  The arguments are gd_receive_turns*'s, then the activation
 * stage's in a struct (device pointers in the device forms, host pointers in the host forms; kind and n_proposed
 * required).
 *   - d_perm / d_offsets, when asked for, are the stable bucketing of the RESOLVED contexts: a message that found
 *     or created its activation lies in that context's bucket in arrival order, not in the null bucket.
 *   - The caller pre-fills state->ctx_flags = GD_CTX_NOT_READY, num_running = 0 and request_count = 0 for every
 *     context it offers in new_ctx / ctx_base...  The turn stage (unchanged) then gives a created activation's
 *     requests GD_TURN_WAIT, in order on its waiting list; a found Invalid one's requests FORWARD /
 *     REJECT_TRANSIENT and its responses RESPONSE / RESPONSE_DROPPED.
 *   - state->hard_limit or hard_limit_stateless_worker > 0: GD_EINVAL.  A null-context closure is enqueued with
 *     a null target, so IncrementEnqueuedOnDispatcherCount never ran for it (IncomingMessageAgent.cs:172-190),
 *     while the turn stage's closed form for EnqueueRequest's hard limit takes every participating message as
 *     counted.  The reference's default is 0 (SiloMessagingOptions.cs:48-67).  With limits on, use gd_activate*
 *     alone and leave those messages' turn to C#.
 *   - frame-fed forms: new_placement is not read; Message.IsNewPlacement comes from the GD_RECV_NULL_CONTEXT
 *     frames themselves (mask bit 18 set and the token SerializationTokenType.True).  A frame left
 *     GD_RECV_UNDECODED never takes part.  ttl_age_ticks and d_msg_flags_or as gd_receive_turns_frames*; rule 1
 *     reads the aged ttl.
 *   - a refused batch: the turn stage still runs (the GD_ACTV_HOST messages keep GD_RECV_NULL_CONTEXT and get
 *     GD_TURN_NONE); the host forms return GD_EINVAL after writing every output. */
typedef struct gd_activate_io {
    const uint8_t*  new_placement;   /* [n] or NULL (array-fed forms)                       */
    int32_t         terminating;
    uint32_t        ctx_base;
    const uint32_t* new_ctx;         /* [cap_new] or NULL                                   */
    uint32_t        cap_new;
    uint8_t*        kind;            /* [n] GD_ACTV_*                                       */
    uint32_t*       new_idx;         /* [n] with n_new, or both NULL                        */
    uint32_t*       n_new;
    uint32_t*       gone_idx;        /* [n] with n_gone, or both NULL                       */
    uint32_t*       n_gone;
    uint32_t*       n_proposed;
} gd_activate_io;
int gd_receive_activate_turns_device(gd_handle* h, const gd_key* d_target_grain, const gd_key* d_target_activation,
                                     const uint8_t* d_direction, uint32_t n, uint32_t n_ctx,
                                     const gd_recv_limits* recv_limits, uint32_t* d_ctx, uint8_t* d_status,
                                     uint32_t* d_perm, uint32_t* d_offsets, const int64_t* d_ttl,
                                     const uint8_t* d_forward_count, const uint8_t* d_msg_flags,
                                     const gd_key* d_sending_activation, const gd_turn_state* state, uint8_t* d_turn,
                                     uint32_t* d_num_running_out, uint32_t* d_running_idx, uint32_t* d_start_idx,
                                     uint32_t* d_n_start, uint32_t* d_wait_perm, uint32_t* d_wait_offsets,
                                     const gd_activate_io* d_act);
int gd_receive_activate_turns(gd_handle* h, const gd_key* target_grain, const gd_key* target_activation,
                              const uint8_t* direction, uint32_t n, uint32_t n_ctx, const gd_recv_limits* recv_limits,
                              uint32_t* out_ctx, uint8_t* out_status, uint32_t* out_perm, uint32_t* out_offsets,
                              const int64_t* ttl, const uint8_t* forward_count, const uint8_t* msg_flags,
                              const gd_key* sending_activation, const gd_turn_state* state, uint8_t* out_turn,
                              uint32_t* out_num_running, uint32_t* out_running_idx, uint32_t* out_start_idx,
                              uint32_t* out_n_start, uint32_t* out_wait_perm, uint32_t* out_wait_offsets,
                              const gd_activate_io* act);
int gd_receive_activate_turns_frames_device(gd_handle* h, const uint8_t* d_buf, uint64_t buf_len,
                                            const uint64_t* d_frame_off, uint32_t n, uint32_t n_ctx,
                                            const gd_recv_limits* recv_limits, const gd_frame_fields* d_out,
                                            const gd_frame_turn_fields* d_turn_out, uint32_t* d_ctx, uint8_t* d_status,
                                            uint32_t* d_perm, uint32_t* d_offsets, int64_t ttl_age_ticks,
                                            const uint8_t* d_msg_flags_or, const gd_turn_state* state, uint8_t* d_turn,
                                            uint32_t* d_num_running_out, uint32_t* d_running_idx, uint32_t* d_start_idx,
                                            uint32_t* d_n_start, uint32_t* d_wait_perm, uint32_t* d_wait_offsets,
                                            const gd_activate_io* d_act);
int gd_receive_activate_turns_frames(gd_handle* h, const uint8_t* buf, uint64_t buf_len, const uint64_t* frame_off,
                                     uint32_t n, uint32_t n_ctx, const gd_recv_limits* recv_limits,
                                     const gd_frame_fields* out, const gd_frame_turn_fields* turn_out, uint32_t* out_ctx,
                                     uint8_t* out_status, uint32_t* out_perm, uint32_t* out_offsets,
                                     int64_t ttl_age_ticks, const uint8_t* msg_flags_or, const gd_turn_state* state,
                                     uint8_t* out_turn, uint32_t* out_num_running, uint32_t* out_running_idx,
                                     uint32_t* out_start_idx, uint32_t* out_n_start, uint32_t* out_wait_perm,
                                     uint32_t* out_wait_offsets, const gd_activate_io* act);

#ifdef __cplusplus
}
#endif
#endif /* GRAINDISPATCH_H */
