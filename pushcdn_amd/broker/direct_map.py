"""The DirectMap: routing hash of a user's public key -> owner, as an
open-addressing table on the device (K5 looks it up every tick) and the host
mirror that decides what goes into it.

  keys / vals   the device table: int64 [S] (bit-cast u64 hash, 0 = empty)
                and int32 [S] (owner; INT32_MIN = tombstone)
  entries       hash -> owner, the source of truth
  pubkeys       hash -> full key: a DIFFERENT key with a registered hash is
                refused, it would take over the other user's Direct traffic
  tombstones    hashes whose key still sits in the device table with a
                tombstoned value (incremental deletes); cleared by a rebuild
  pending       the DirectMap half of the engine's membership log: hash ->
                (owner or None for a delete, whether the device table held
                the hash before the first pending change)

Every registration is admitted (_admit: hash, collision, hash 0) and checked
for room (_check_room) before the dicts change, and the dicts change before
the device hears of it, so a refusal leaves host and device as they were.  The device follows by a
whole-table rebuild (register / unregister), one incremental apply (update)
or at the next flush (queue_upsert / queue_delete).
"""

from __future__ import annotations

from typing import Callable, Dict, List, Optional, Tuple

import torch

from ..ops.reference import build_direct_table
from ..utils.keyhash import fnv1a64
from ..utils.log import get_logger

log = get_logger("direct-map")

_NOTHING: Dict[int, Tuple[bytes, int]] = {}


class DirectMap:
    def __init__(self, size: int, device: torch.device, hash_seed: int,
                 apply: Callable[[torch.Tensor, torch.Tensor, List[Tuple[int, int]],
                                  List[int]], int]) -> None:
        """apply(keys, vals, up_list, dels) -> failed: the incremental device
        update (K6 or its model) with (hash, owner) upserts and hashes to
        tombstone, all distinct; returns how many upserts found no slot."""
        self.size = size
        self.keys = torch.zeros(size, dtype=torch.int64, device=device)
        self.vals = torch.zeros(size, dtype=torch.int32, device=device)
        self.hash_seed = hash_seed
        self.entries: Dict[int, int] = {}
        self.pubkeys: Dict[int, bytes] = {}
        self.tombstones: set = set()
        self.pending: Dict[int, Tuple[Optional[int], bool]] = {}
        self._apply = apply

    # ------------------------------ admission ------------------------------

    def _admit(self, pubkey: bytes, staged: Dict[int, Tuple[bytes, int]] = _NOTHING) -> int:
        """Routing hash of a key that may be registered.  `staged` holds the
        keys this call admitted before it.  If a DIFFERENT pubkey holds the
        same 64-bit hash, registering this one would silently misroute one
        user's Direct traffic to the other: refuse (accidental probability
        2^-64 per pair; adversarial construction requires the secret seed).
        Hash 0 is the table's empty marker."""
        h = fnv1a64(pubkey, self.hash_seed)
        prev = self.pubkeys.get(h)
        if prev is None and h in staged:
            prev = staged[h][0]
        if prev is not None and prev != pubkey:
            raise ValueError("direct routing-hash collision with a different registered key")
        if h == 0:
            raise ValueError("routing hash 0 is the empty marker; not registered")
        return h

    def _owned(self, pubkey: bytes) -> Optional[int]:
        """The hash of `pubkey` while its entry still belongs to that key."""
        h = fnv1a64(pubkey, self.hash_seed)
        return h if h in self.entries and self.pubkeys.get(h) == pubkey else None

    def _check_room(self, new: int, freed: int = 0) -> None:
        """`new` hashes the dicts do not hold, `freed` that they will drop."""
        if len(self.entries) - freed + new > self.size:
            raise RuntimeError("direct table full")

    def _commit(self, ups: Dict[int, Tuple[bytes, int]], dels=()) -> None:
        """Write admitted upserts and owned deletes (distinct hashes) to the
        host dicts, or raise before anything changes if the live entries
        would not fit the table."""
        entries, pubkeys = self.entries, self.pubkeys
        self._check_room(sum(1 for h in ups if h not in entries), len(dels))
        for h in dels:
            del entries[h]
            del pubkeys[h]
        for h, (pubkey, owner) in ups.items():
            entries[h] = owner
            pubkeys[h] = pubkey

    # ------------------------- immediate: by rebuild -------------------------

    def register(self, entries) -> None:
        """Register (pubkey, owner) pairs, all or none, with one rebuild."""
        ups: Dict[int, Tuple[bytes, int]] = {}
        for pubkey, owner in entries:
            ups[self._admit(pubkey, ups)] = (pubkey, owner)
        self._commit(ups)
        self.rebuild()

    def unregister(self, pubkey: bytes) -> None:
        h = fnv1a64(pubkey, self.hash_seed)
        if self.entries.pop(h, None) is not None:
            self.pubkeys.pop(h, None)
            self.rebuild()

    def rebuild(self) -> None:
        keys, vals = build_direct_table(list(self.entries.items()), self.size)
        self.keys.copy_(keys.to(self.keys.device))
        self.vals.copy_(vals.to(self.vals.device))
        self.tombstones.clear()

    def keys_owned_by(self, owner: int) -> List[bytes]:
        return [self.pubkeys[h] for h, o in self.entries.items() if o == owner]

    # --------------------- immediate: one incremental apply ---------------------

    def update(self, upserts, deletes) -> None:
        """See GpuBrokerEngine.apply_direct_updates."""
        ups: Dict[int, Tuple[bytes, int]] = {}
        for pubkey, owner in upserts:
            try:
                ups[self._admit(pubkey, ups)] = (pubkey, int(owner))
            except ValueError as e:
                log.warning("%s; skipping remote entry", e)
        dels: Dict[int, None] = {}   # insertion-ordered set
        for pubkey in deletes:
            h = self._owned(pubkey)
            if h is not None and h not in ups:
                dels[h] = None
        dels = list(dels)
        self._commit(ups, dels)
        self._push([(h, o) for h, (_k, o) in ups.items()], dels)

    # ------------------------------ the log half ------------------------------

    # One key per call, once per connect and disconnect: written out, not
    # through _commit.  pending[h] remembers whether the device table held
    # the hash before the first pending change (the dicts did, then), so a
    # delete of an entry that never reached the device is dropped at flush.

    def queue_upsert(self, pubkey: bytes, owner: int) -> None:
        h = self._admit(pubkey)
        held = h in self.entries
        if not held:
            self._check_room(1)
        prev = self.pending.get(h)
        self.pending[h] = (owner, prev[1] if prev is not None else held)
        self.entries[h] = owner
        self.pubkeys[h] = pubkey

    def queue_delete(self, pubkey: bytes) -> None:
        """Deletes the entry only while it still belongs to `pubkey`."""
        h = self._owned(pubkey)
        if h is not None:
            prev = self.pending.get(h)
            self.pending[h] = (None, prev[1] if prev is not None else True)
            del self.entries[h]
            del self.pubkeys[h]

    def flush(self) -> None:
        if self.pending:
            pending, self.pending = self.pending, {}
            self._push([(h, o) for h, (o, _dev) in pending.items() if o is not None],
                       [h for h, (o, on_device) in pending.items() if o is None and on_device])

    # -------------------------------- device --------------------------------

    def _push(self, up_list: List[Tuple[int, int]], dels: List[int]) -> None:
        """Bring the device table in line with the host dicts, which already
        hold the change.  One incremental apply, or a rebuild where the
        tombstone rule or a failed insert asks for one."""
        if not up_list and not dels:
            return
        tombstones = (self.tombstones | set(dels)) - {h for h, _ in up_list}
        # slots in use once this batch is in: live entries + tombstones
        used = len(self.entries) + len(tombstones)
        # compaction reclaims tombstoned slots only: with none, a table past
        # half full keeps taking incremental inserts (probe chains grow, as
        # in any open-addressing table; size gpu_direct_table_size at twice
        # the cluster's users to stay below it) and falls back to the
        # rebuild through the failed count
        if used > self.size // 2 and tombstones:
            self.rebuild()
            return
        self.tombstones = tombstones
        try:
            failed = self._apply(self.keys, self.vals, up_list, dels)
        except Exception:
            # the host dicts already hold the update: bring the device table
            # back in line with them before the error travels on
            self.rebuild()
            raise
        if failed:   # an insert found no slot
            self.rebuild()
