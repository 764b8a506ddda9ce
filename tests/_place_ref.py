"""Restatement of the placement of unregistered grains (Dispatcher.AddressMessageAsync's slow path) for
the gd_route_place tests, written from the reference's source:

  src/Orleans.Runtime/Core/Dispatcher.cs:742-767                          AddressMessageAsync: SelectOrAddActivation,
                                                                          SetTargetPlacement, IsNewPlacement
  src/Orleans.Runtime/Placement/PlacementDirectorsManager.cs:79-116       SelectOrAddActivation, AddActivation
  src/Orleans.Runtime/Placement/HashBasedPlacementDirector.cs:11-14       OnAddActivation
  src/Orleans.Runtime/Placement/PreferLocalPlacementDirector.cs:17-26     OnAddActivation
  src/Orleans.Runtime/Placement/ActivationCountPlacementDirector.cs:89-122, RandomPlacementDirector
                                                                          (the choice draws SafeRandom: made in C#)
  src/Orleans.Runtime/GrainDirectory/GrainDirectoryPartition.cs:304-326   AddSingleActivation (IsValidSilo :310)
  src/Orleans.Core.Abstractions/IDs/SiloAddress.cs:280-329                CompareTo (the HASH order)

Two forms: place_loop, a literal per-message loop over an oracle.dirstate.DirectoryState, and place_np,
the same vectorised for the larger sizes.  Both take the route's outputs (status, silo, act) for the
directory as it was before the batch, change the directory, and return
(status u8[n], silo u32[n], act u32[n], placed u8[n], new_idx u32[n_new], n_proposed)."""
import functools

import numpy as np

import oracle as o
from dirstate import version_tag

PLACE_NONE, PLACE_HASH, PLACE_LOCAL, PLACE_GIVEN = range(4)
PLACED_NONE, PLACED_NEW, PLACED_JOINED, PLACED_SKIPPED = range(4)
NO_SILO = 0xFFFFFFFF
ACT_MULTI = 0xFFFFFFFE


class PlaceConfig:
    """What gd_place_configure holds: the silo table, the compatible flags (context.GetCompatibleSilos) and
    whether the local silo is Active.  compare(a, b): SiloAddress.CompareTo over two table entries."""

    def __init__(self, silos, compatible=None, local_active=True, my_silo=0, compare=None):
        self.silos = list(silos)
        n = len(self.silos)
        self.n_silos = n
        self.compatible = [True] * n if compatible is None else [bool(x) for x in compatible]
        self.local_active = bool(local_active)
        self.my_silo = my_silo
        cmp = compare or (lambda a, b: a.compare_to(b))
        # HashBasedPlacementDirector.cs:11  context.GetCompatibleSilos(target).OrderBy(s => s).ToArray()
        self.sorted = sorted([s for s in range(n) if self.compatible[s]],
                             key=functools.cmp_to_key(lambda x, y: cmp(self.silos[x], self.silos[y])))


def choose_silo(key, strategy, given, cfg):
    """The silo the strategy's director returns for one new grain, or None (no placement here)."""
    if strategy == PLACE_HASH:
        # HashBasedPlacementDirector.cs:12  int hash = (int)(GetUniformHashCode() & 0x7fffffff);
        h = o.jenkins_u64x3(key[2], key[0], key[1]) & 0x7FFFFFFF
        return cfg.sorted[h % len(cfg.sorted)]              # :14  allSilos[hash % allSilos.Length]
    if strategy == PLACE_LOCAL:
        # PreferLocalPlacementDirector.cs:21  if (LocalSiloStatus != Active || !compatible.Contains(LocalSilo))
        local_ok = cfg.local_active and cfg.my_silo < cfg.n_silos and cfg.compatible[cfg.my_silo]
        if local_ok:
            return cfg.my_silo                               # :24-25
        return given                                         # :22 base.OnAddActivation: random, drawn in C#
    if strategy == PLACE_GIVEN:                              # RandomPlacement / ActivationCountPlacement: C#'s draw
        return given
    return None                                              # PLACE_NONE, or no known value


def place_one(key, strategy, given, cfg, directory):
    """('none' | 'skip' | 'place', silo) for one message the route left MISS."""
    if o.category_of(key[2]) != o.CAT_GRAIN:                 # PlacementDirectorsManager.cs:85-93,108-109: clients
        return "none", None                                  # (and everything else that is no plain grain)
    if not cfg.sorted:                                       # no compatible silo
        return "skip", None
    s = choose_silo(key, strategy, given, cfg)
    if s is None or s >= cfg.n_silos or not cfg.compatible[s]:
        return "skip", None
    if not directory.silo_valid(s):                          # GrainDirectoryPartition.cs:310  IsValidSilo
        return "skip", None
    return "place", s


def _strategy_at(strategy, i):
    return int(strategy) if np.isscalar(strategy) else int(strategy[i])


def place_loop(keys, route, strategy, given, act_base, cfg, directory):
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
    status, silo, act = (np.array(a, copy=True) for a in route)
    n = len(keys)
    placed = np.zeros(n, np.uint8)
    new_idx = []
    c = 0
    directory.op += 1                                        # one mutating directory call (VersionTag numbering)
    for i in range(n):
        if status[i] != o.ST_MISS:                           # Dispatcher.cs:718-741: addressed, or not the directory's
            continue
        k = tuple(int(x) for x in keys[i])
        what, s = place_one(k, _strategy_at(strategy, i), None if given is None else int(given[i]), cfg, directory)
        if what == "none":
            continue
        if what == "skip":
            placed[i] = PLACED_SKIPPED
            continue
        proposal = act_base + c
        c += 1
        e = directory.entries.get(k)
        if e is None:                                        # GrainDirectoryPartition.cs:312-325: first wins
            directory.entries[k] = [proposal, s, version_tag(directory.op, k), True]
            status[i], silo[i], act[i], placed[i] = o.ST_OK, s, proposal, PLACED_NEW    # Dispatcher.cs:753-767
            new_idx.append(i)
        else:                                                # the registered address comes back
            status[i], silo[i], act[i], placed[i] = o.ST_OK, e[1], e[0], PLACED_JOINED
    return status, silo, act, placed, np.array(new_idx, dtype=np.uint32), c


def place_np(keys, route, strategy, given, act_base, cfg, directory):
    keys = np.asarray(keys, dtype=np.uint64).reshape(-1, 3)
    status, silo, act = (np.array(a, copy=True) for a in route)
    n = len(keys)
    placed = np.zeros(n, np.uint8)
    strat = np.full(n, int(strategy), np.uint8) if np.isscalar(strategy) else np.asarray(strategy, dtype=np.uint8)
    cat = (keys[:, 2] >> np.uint64(56)).astype(np.uint32)
    cand = (status == o.ST_MISS) & (cat == o.CAT_GRAIN)
    chosen = np.full(n, NO_SILO, np.int64)
    if cfg.sorted:
        srt = np.asarray(cfg.sorted, dtype=np.int64)
        h = o.jenkins_u64x3_np(keys[:, 2], keys[:, 0], keys[:, 1]).astype(np.int64) & 0x7FFFFFFF
        chosen = np.where(strat == PLACE_HASH, srt[h % len(srt)], chosen)
        gv = np.full(n, NO_SILO, np.int64) if given is None else np.asarray(given, dtype=np.uint32).astype(np.int64)
        local_ok = cfg.local_active and cfg.my_silo < cfg.n_silos and cfg.compatible[cfg.my_silo]
        chosen = np.where(strat == PLACE_LOCAL, cfg.my_silo if local_ok else gv, chosen)
        chosen = np.where(strat == PLACE_GIVEN, gv, chosen)
    in_range = chosen < cfg.n_silos
    safe = np.where(in_range, chosen, 0)
    compat = np.asarray(cfg.compatible, dtype=bool)
    valid = np.array([directory.silo_valid(s) for s in range(cfg.n_silos)], dtype=bool)
    placing = cand & in_range & compat[safe] & valid[safe]
    placed[cand & ~placing] = PLACED_SKIPPED
    pi = np.flatnonzero(placing)
    proposal = act_base + np.arange(len(pi), dtype=np.int64)
    directory.op += 1
    new_idx = np.zeros(0, np.uint32)
    if len(pi):
        kv = o._key_void(keys[pi])
        _, first, inv = np.unique(kv, return_index=True, return_inverse=True)
        win_act = np.zeros(len(first), np.int64)
        win_silo = np.zeros(len(first), np.int64)
        created = np.zeros(len(first), bool)
        for u, f in enumerate(first):                        # one AddSingleActivation per distinct grain
            k = tuple(int(x) for x in keys[pi[f]])
            e = directory.entries.get(k)
            if e is None:
                e = directory.entries[k] = [int(proposal[f]), int(chosen[pi[f]]), version_tag(directory.op, k), True]
                created[u] = True
            win_act[u], win_silo[u] = e[0], e[1]
        is_new = created[inv] & (first[inv] == np.arange(len(pi)))
        status[pi] = o.ST_OK
        silo[pi] = win_silo[inv].astype(np.uint32)
        act[pi] = win_act[inv].astype(np.uint32)
        placed[pi] = np.where(is_new, PLACED_NEW, PLACED_JOINED)
        new_idx = pi[is_new].astype(np.uint32)
    return status, silo, act, placed, new_idx, len(pi)


def route_of(keys, spec, directory, my_silo, seed_silo):
    """gd_route's (status, silo, act) for the directory as it is."""
    st, silo, act, _, _ = o.route_batch_np(keys, spec, o.DirectoryArrays(*directory.as_arrays()), my_silo=my_silo,
                                           seed_silo=seed_silo)
    return st, silo, act


def mixed_keys(rng, n, type_code, n_grains, new_share=0.3):
    """n target keys over n_grains registered-or-not plain grains (ids below n_grains are the registered ones;
    ids at or above are new, drawn from a small range so that new grains repeat in the batch), with client,
    KeyExt and system targets and the membership grain mixed in."""
    ids = rng.integers(0, n_grains, size=n)
    new = rng.random(n) < new_share
    ids[new] = n_grains + rng.integers(0, max(1, n // 8), size=int(new.sum()))
    keys = o.grain_keys(type_code, ids)
    special = np.zeros((4, 3), np.uint64)
    special[0] = (0, 9, o.type_code_data(o.CAT_SYSTEM_TARGET, 12))
    special[1] = (0, 5, o.type_code_data(o.CAT_KEYEXT_GRAIN, type_code))
    mt = o.MEMBERSHIP_TABLE_ID
    special[2] = (mt.n0, mt.n1, mt.tcd)
    special[3] = (7, 11, o.type_code_data(o.CAT_CLIENT, 0))
    m = n // 10
    if m:
        keys[rng.choice(n, size=m, replace=False)] = special[rng.integers(0, 4, size=m)]
    return keys
