"""The GPU broker data-plane engine (one instance per MI355X device).

Owns the HBM-resident state and drives the kernel pipeline per tick:

    ingest (H2D pinned staging)          [reference: per-conn reader tasks]
      -> K4 parse_batch                  [message.rs deserialize]
      -> K2a topic_mask                  [connections get_interested_by_topic]
      -> (mesh all-gather via RCCL)      [try_send_to_brokers over xGMI]
      -> K2b assign_emit                 [per-conn FIFO channel push]
      -> K3 fanout                       [sender.rs raw-bytes fan-out copy]
      -> K5 direct_lookup                [DirectMap get]

State tensors (all owned by PyTorch, sized for 288 GB HBM):
  sub_bitmap  int64 [256][W]      subscription bitmap (W = ceil(R/64))
  egress      uint8 [R*ring_bytes]  per-recipient egress rings
  ring_wpos   int64 [R]           ring write cursors (device)
  direct_keys/vals                open-addressing DirectMap (u64 hash -> owner)

R = n_users + n_peer_slots: recipients [0, n_users) are local users,
recipient n_users + p is peer broker slot p (DirectMap owner -(p+2)).

Delivery record format in a ring: {u32 len, u32 seq, u64 pad} + payload,
16-byte aligned.  A drain (the socket-write analog) reads the cursors back,
consumes records, and resets the cursors.

By-reference delivery (ref_threshold set): a message of at least
ref_threshold wire bytes is delivered as a bare 16-byte record
{u32 len | 0x80000000, u32 seq, u64 ref_off}; its bytes stay in the host
batch, which the engine retains and drain_compact_ref() hands back as the
reference buffer ref_off indexes.

Loss accounting (loss_accounting=True): a delivery that does not fit its
ring, or finds the pair list full, is dropped on the device.  A second
per-recipient accumulator, demand (int64 [R]), takes the ring bytes every
tick WANTED to deliver (K9); at a drain demand[r] - ring_wpos[r] is what
recipient r lost (K10), reported by take_losses().

Framed drain (drain_framed): K11 hands every recipient's records over as
socket-ready [u32 big-endian len][message] frames in seq order instead of raw
ring records, so the host neither parses nor sorts nor re-copies them.

CPU mode (device="cpu") runs the pure-Python mirrors from ops.reference so
the engine's semantics are testable without a GPU.
"""

from __future__ import annotations

import os

from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np
import torch

from ..ops import reference as ref
# the ring record format is re-exported: callers import it from here
from ..ops.ring_format import (FRAME_SORT_MAX, RING_ALIGN, REF_FLAG,  # noqa: F401
                               parse_frames, parse_ring_records, ring_rec)
from ..utils.keyhash import as_i64
from .direct_map import DirectMap


def _k6_apply(ops, device):
    """The DirectMap's incremental device update on the GPU plane, as the
    callable DirectMap takes: one K6 launch per call."""
    n_failed = torch.zeros(1, dtype=torch.int32, device=device)

    def apply(keys, vals, up_list, dels) -> int:
        up_keys = torch.tensor([as_i64(h) for h, _ in up_list], dtype=torch.int64).to(device)
        up_owners = torch.tensor([o for _, o in up_list], dtype=torch.int32).to(device)
        del_keys = torch.tensor([as_i64(h) for h in dels], dtype=torch.int64).to(device)
        ops.direct_apply(keys, vals, up_keys, up_owners, del_keys, n_failed)
        # A 4-byte readback, also on a tick whose membership flush carries
        # DirectMap changes: an insert that found no slot has to be repaired
        # by a rebuild BEFORE that tick's K5 looks the key up.
        failed = int(n_failed.cpu()[0])
        if failed:
            n_failed.zero_()
        return failed

    return apply


@dataclass
class TickStats:
    n_messages: int = 0
    n_broadcast: int = 0
    n_direct: int = 0
    n_deliveries: int = 0
    n_drops: int = 0


class GpuBrokerEngine:
    def __init__(
        self,
        device: str = "cuda:0",
        n_users: int = 10_000,
        ring_bytes: int = 1 << 21,
        direct_table_size: int = 1 << 16,
        use_gpu_ops: Optional[bool] = None,
        fanout_wire: bool = False,
        pair_capacity: int = 4 << 20,
        nt_fanout: bool = True,
        direct_enabled: bool = True,
        hash_seed: int = 0,
        n_peer_slots: int = 0,
        ref_threshold: Optional[int] = None,
        fused_tick: bool = True,
        loss_accounting: bool = False,
    ) -> None:
        # n_peer_slots (P): peer brokers as recipients of the device
        # pipeline.  The recipient index space is R = n_users + P; peer slot
        # p is recipient n_users + p with its own egress ring, and owner
        # value -(p+2) in the DirectMap.  A peer takes each message at most
        # once per tick, like a user subscribed to the peer's topics, so
        # K2b / K3 / K7 serve it unchanged.  n_users stays the LOCAL users.
        assert n_peer_slots >= 0
        self.n_peer_slots = n_peer_slots
        self.n_recipients = n_users + n_peer_slots
        # pair_capacity bounds the preallocated delivery-pair buffers (the
        # sync-free pipeline drops + counts beyond it); nt_fanout uses
        # non-temporal egress stores; direct_enabled can be turned off for
        # broadcast-only workloads to skip the per-tick K5 host check.
        self.pair_capacity = pair_capacity
        # flat-vs-wave fan-out cutover (bytes/record): flat wins on small
        # records (wave idles tail lanes), wave won by ~3% at >=4 KiB
        # before the magic-division address math — env knob for A/B
        self._flat_max_rec = int(os.environ.get("PUSHCDN_FLAT_MAX_REC", "4096"))
        # the flat kernel's unit index is a u32 with an exact magic division
        # only for units_per_pair <= 2^21 and capacity * units < 2^31 (the
        # bindings check the same per launch) — fail a bad config here
        flat_units = self._flat_max_rec // 16 + 1
        assert 1 <= flat_units <= (1 << 21), "PUSHCDN_FLAT_MAX_REC too large"
        assert pair_capacity * flat_units < (1 << 31), (
            f"pair_capacity {pair_capacity} x {flat_units} flat units/record "
            "must stay below 2^31")
        self.nt_fanout = nt_fanout
        self.direct_enabled = direct_enabled
        # fused_tick: a uniform broadcast-only tick (see _fused_tick_ok) runs
        # as one native call, and drain_cursors as one; False keeps the
        # per-op path everywhere.  fused_ticks counts the ticks that took it.
        self.fused_tick = fused_tick
        self.fused_ticks = 0
        # hash_seed keys the routing hash (keyhash.derive_routing_seed from
        # the cluster private key in live services): without it FNV-1a
        # collisions are offline-grindable and a crafted pubkey could siphon
        # a victim's Direct messages (K5 matches on the 64-bit hash only).
        self.hash_seed = hash_seed & ((1 << 64) - 1)
        # fanout_wire=True: fan out the WHOLE serialized wire message (the
        # reference's raw-bytes-forwarded-verbatim invariant);
        # False: fan out only the payload field (kernel golden tests).
        self.fanout_wire = fanout_wire
        self.device = torch.device(device)
        self.is_cuda = self.device.type == "cuda"
        if use_gpu_ops is None:
            use_gpu_ops = self.is_cuda
        self.use_gpu_ops = use_gpu_ops
        if self.use_gpu_ops:
            from ..ops import get_gpu_ops

            self._ops = get_gpu_ops()
        else:
            self._ops = None

        assert ring_bytes % 16 == 0
        self.n_users = n_users
        self.ring_bytes = ring_bytes
        R = self.n_recipients
        self.W = (R + 63) // 64

        dev = self.device
        self.sub_bitmap = torch.zeros((256, self.W), dtype=torch.int64, device=dev)
        self.egress = torch.zeros(R * ring_bytes, dtype=torch.uint8, device=dev)
        self.ring_wpos = torch.zeros(R, dtype=torch.int64, device=dev)
        # the DirectMap (device table + host mirror); the CPU model is looked
        # up per call
        self.directs = DirectMap(
            direct_table_size, dev, self.hash_seed,
            _k6_apply(self._ops, dev) if self.use_gpu_ops
            else lambda *args: ref.direct_apply(*args))
        self.direct_keys = self.directs.keys
        self.direct_vals = self.directs.vals
        # the membership log (see queue_join): recipient -> [clear, set, reset]
        # with 256-bit topic sets as ints; its DirectMap half is directs.pending
        self._mship_rows: Dict[int, list] = {}
        self._ctl_ops = None  # pushcdn_gpu_ctl, loaded by the first flush
        # by-reference delivery (None = off: exactly the inline kernels).
        # Needs fanout_wire, so that host and device both know a message's
        # fanned-out length from the batch offsets alone; every message
        # that stays inline must fit an empty ring.
        if ref_threshold is not None:
            assert fanout_wire, "ref_threshold requires fanout_wire=True"
            assert 1 <= ref_threshold < REF_FLAG
            assert ring_rec(ref_threshold - 1) <= ring_bytes, (
                f"ref_threshold {ref_threshold}: an inline message just below it "
                f"does not fit a {ring_bytes}-byte ring")
        self.ref_threshold = ref_threshold
        # host batches that undrained by-reference records point into, in
        # tick order, and their total size (the next batch's ref_base)
        self._ref_batches: List[bytes] = []
        self._ref_base = 0
        # loss accounting (False = off: nothing allocated, no extension
        # loaded, not one extra launch or copy).  demand[r] accumulates the
        # ring bytes the ticks wanted to deliver to r since the last drain,
        # ring_wpos[r] is what they did deliver, and every drain reports the
        # recipients where the two differ (take_losses).  That covers a full
        # ring and a full pair list alike.
        self.loss_accounting = loss_accounting
        self._acct_ops = None
        self._losses: Dict[int, int] = {}
        if loss_accounting:
            self.demand = torch.zeros(R, dtype=torch.int64, device=dev)
            if self.use_gpu_ops:
                from ..ops import get_gpu_acct_ops

                self._acct_ops = get_gpu_acct_ops()
                # K10's outputs: the (recipient, bytes) list, its length on
                # the device and in pinned host memory
                self._lossy = torch.empty((max(R, 1), 2), dtype=torch.int64, device=dev)
                self._n_lossy = torch.zeros(1, dtype=torch.int32, device=dev)
                self._n_lossy_host = torch.zeros(1, dtype=torch.int32,
                                                 pin_memory=self.is_cuda)
        self.seq = 0
        self.total = TickStats()
        # drain_compact's device staging and its two pinned host buffers;
        # _staging_flip is the host buffer the next drain fills
        self._staging_dev: Optional[torch.Tensor] = None
        self._staging_host: Optional[List[torch.Tensor]] = None
        self._staging_flip = 0
        # drain_framed's extras, made by its first call: the extension, K11's
        # record index (as large as the device staging) and the per-recipient
        # frame_len / frame_cnt on the device and in pinned host memory
        self._drain_ops = None
        self._frame_index: Optional[torch.Tensor] = None
        self._frame_meta = None
        self._k2b_scratch = None  # (blocks it serves, block-K2b buffers)
        if self.use_gpu_ops:
            o32 = dict(dtype=torch.int32, device=dev)
            # delivery pairs as 16 B AoS records {i32 user, i32 msg, i64 dst}
            # — one dword4 store per pair in the emitters, one dword4 load
            # per unit in K3 (SoA cost 3x scattered sub-line stores)
            self._pairs = torch.empty((pair_capacity, 4), **o32)
            self._drops = torch.zeros(1, **o32)
            self._n_pairs = torch.zeros(1, **o32)
            self._seq_dev = torch.zeros(1, **o32)  # device seq counter (graph path)
            # fused tick: length of the sparse pair list of the last tick
            self._n_sparse = torch.zeros(1, **o32)
            self._dense_fanout = True
            self._fused_scratch = None
            self._fused_scratch_shape = None  # (M, W, wire length) it was last sized for
            self._drain_bufs = None
            self._graphs: Dict[Tuple[int, int, int], object] = {}

    # ---------------- subscription management (host-driven) ----------------

    @staticmethod
    def _word_bit(recipient: int) -> Tuple[int, int]:
        """Bitmap word index and (int64) bit of a recipient."""
        return recipient >> 6, as_i64(1 << (recipient & 63))

    def subscribe(self, user_idx: int, topics: List[int]) -> None:
        self.flush_membership()
        w, bit = self._word_bit(user_idx)
        for t in topics:
            self.sub_bitmap[t & 0xFF, w] |= bit

    def unsubscribe(self, user_idx: int, topics: List[int]) -> None:
        self.flush_membership()
        w, bit = self._word_bit(user_idx)
        for t in topics:
            self.sub_bitmap[t & 0xFF, w] &= ~bit

    def subscribe_all(self, topics: List[int]) -> None:
        """Subscribe every user to the given topics (bulk, for benches)."""
        self.flush_membership()
        if self.n_peer_slots:
            # user bits only: peer-slot bits of the row are kept
            full = self._user_bit_words().to(self.device)
            for t in topics:
                self.sub_bitmap[t & 0xFF] |= full
            return
        full = torch.full((self.W,), -1, dtype=torch.int64)
        tail = self.n_users & 63
        if tail:
            full[-1] = (1 << tail) - 1
        for t in topics:
            self.sub_bitmap[t & 0xFF] = full.to(self.device)

    def _user_bit_words(self) -> torch.Tensor:
        """int64 [W]: the bits of every bitmap word that belong to local
        users (recipients below n_users)."""
        words = torch.zeros(self.W, dtype=torch.int64)
        nfull = self.n_users >> 6
        words[:nfull] = -1
        tail = self.n_users & 63
        if tail:
            words[nfull] = (1 << tail) - 1
        return words

    # ------------------------------ peer slots ------------------------------

    def _peer_word_bit(self, p: int) -> Tuple[int, int]:
        if not 0 <= p < self.n_peer_slots:
            raise IndexError(f"peer slot {p} outside [0, {self.n_peer_slots})")
        return self._word_bit(self.n_users + p)

    def set_peer_topics(self, p: int, topics: List[int]) -> None:
        """Make `topics` the exact interest set of peer slot p: a local
        Broadcast on any of them lands once in ring n_users + p."""
        self.flush_membership()
        w, bit = self._peer_word_bit(p)
        self.sub_bitmap[:, w] &= ~bit
        rows = sorted({t & 0xFF for t in topics})
        if rows:
            self.sub_bitmap[torch.tensor(rows, device=self.device), w] |= bit

    def clear_peer(self, p: int) -> None:
        """Release peer slot p: no topic reaches its ring any more and
        whatever the ring still holds is discarded.  Its DirectMap entries
        are the caller's to delete (direct_keys_owned_by +
        apply_direct_updates)."""
        self.flush_membership()
        w, bit = self._peer_word_bit(p)
        self.sub_bitmap[:, w] &= ~bit
        self.ring_wpos[self.n_users + p] = 0
        if self.loss_accounting:
            # cursor and demand are reset together: the slot's next occupant
            # must not inherit a loss
            self.demand[self.n_users + p] = 0

    def register_direct(self, pubkey: bytes, owner: int) -> None:
        """owner >= 0: local user index. owner <= -2: peer slot -(p+2).
        Raises ValueError on a routing-hash collision with a different
        registered key (or routing hash 0) and RuntimeError("direct table
        full"); a refusal changes nothing."""
        self.flush_membership()
        self.directs.register([(pubkey, owner)])

    def register_direct_bulk(self, entries) -> None:
        """Register many (pubkey, owner) pairs with one table rebuild, or
        none of them if one is refused."""
        self.flush_membership()
        self.directs.register(entries)

    def unregister_direct(self, pubkey: bytes) -> None:
        """Remove a departed user's entry so a Direct to their key is dropped
        instead of delivered to whoever reuses the slot."""
        self.flush_membership()
        self.directs.unregister(pubkey)

    def subscribe_modulo(self, n_topics: int) -> None:
        """Bulk: user u subscribes to topic (u % n_topics) — the mixed-bench
        population shape. Vectorized bitmap build on host, one H2D copy."""
        self.flush_membership()
        bitmap = np.zeros((256, self.W), dtype=np.uint64)
        users = np.arange(self.n_users)
        for t in range(n_topics):
            sel = users[users % n_topics == t]
            words = sel >> 6
            bits = np.zeros(self.W, dtype=np.uint64)
            np.bitwise_or.at(bits, words, np.uint64(1) << (sel & 63).astype(np.uint64))
            bitmap[t] = bits
        new = torch.from_numpy(bitmap.view(np.int64)).to(self.device)
        if self.n_peer_slots:
            # user bits only: carry the peer-slot bits over
            new |= self.sub_bitmap & ~self._user_bit_words().to(self.device)
        self.sub_bitmap.copy_(new)

    def direct_keys_owned_by(self, owner: int) -> List[bytes]:
        """Pubkeys whose DirectMap entry currently holds `owner`."""
        return self.directs.keys_owned_by(owner)

    def apply_direct_updates(self, upserts, deletes) -> None:
        """Batched incremental DirectMap update: `upserts` is a list of
        (pubkey, owner), `deletes` a list of pubkeys.  One K6 launch (or the
        CPU mirror) instead of a host rebuild + two table copies.

        The host dicts stay the source of truth.  Within one call the last
        upsert of a key wins, and an upsert wins over a delete of the same
        key.  An entry whose hash collides with a DIFFERENT registered key,
        or is 0, is skipped and logged (remote entries must not raise).
        Deletes tombstone the value and leave the key in its slot; when live
        + tombstoned slots would pass half the table and there is a tombstone
        to reclaim, or the kernel reports an update that found no slot, the
        table is compacted by a rebuild.
        Raises RuntimeError("direct table full") if the live entries alone
        do not fit."""
        self.flush_membership()
        self.directs.update(upserts, deletes)

    # ---------------------------- membership log ----------------------------
    #
    # queue_* record user joins, leaves and subscription changes on the host;
    # flush_membership() applies everything pending with one K8 launch
    # (bitmap bits + ring cursors) and one K6 launch (DirectMap).  The log is
    # kept COALESCED: one row (clear, set, reset) per recipient and one
    # pending upsert/delete per routing hash, folded in program order, so it
    # never holds more than n_recipients rows whatever the churn.  tick(),
    # tick_graphed(), every drain_* and every immediate state-changing method
    # flush first, so mixed use keeps program order.

    _ALL_TOPICS = (1 << 256) - 1

    @property
    def pending_membership(self) -> int:
        """Rows the next flush_membership() will apply."""
        return len(self._mship_rows)

    @staticmethod
    def _topic_bits(topics) -> int:
        bits = 0
        for t in topics:
            bits |= 1 << (t & 0xFF)
        return bits

    def _check_recipient(self, r: int, limit: int) -> None:
        if not 0 <= r < limit:
            raise IndexError(f"recipient {r} outside [0, {limit})")

    def _queue_row(self, r: int, clear: int, set_: int, replace: bool) -> None:
        row = self._mship_rows.get(r)
        if replace:
            # join / leave: whatever was pending for r is superseded
            self._mship_rows[r] = [self._ALL_TOPICS, set_, True]
        elif row is None:
            self._mship_rows[r] = [clear, set_, False]
        else:
            row[0] = (row[0] | clear) & ~set_
            row[1] = (row[1] | set_) & ~clear

    def queue_subscribe(self, recipient: int, topics: List[int]) -> None:
        self._check_recipient(recipient, self.n_recipients)
        self._queue_row(recipient, 0, self._topic_bits(topics), False)

    def queue_unsubscribe(self, recipient: int, topics: List[int]) -> None:
        self._check_recipient(recipient, self.n_recipients)
        self._queue_row(recipient, self._topic_bits(topics), 0, False)

    def queue_join(self, slot: int, pubkey: bytes, topics: List[int]) -> None:
        """A user takes `slot`: its interest becomes exactly `topics`, its
        ring cursor is reset, hash(pubkey) -> slot is upserted.  Raises
        ValueError on a routing-hash collision with a different registered
        key (or routing hash 0) and RuntimeError when the DirectMap is full;
        a refusal leaves the log and the host dicts untouched."""
        self._check_recipient(slot, self.n_users)
        self.directs.queue_upsert(pubkey, slot)
        self._queue_row(slot, 0, self._topic_bits(topics), True)

    def queue_leave(self, slot: int, pubkey: Optional[bytes]) -> None:
        """The user of `slot` departs: all 256 topics cleared, the cursor
        reset, and the DirectMap entry deleted if it still belongs to
        `pubkey` (None: no entry to delete)."""
        self._check_recipient(slot, self.n_users)
        if pubkey is not None:
            self.directs.queue_delete(pubkey)
        self._queue_row(slot, 0, 0, True)

    def flush_membership(self) -> None:
        """Apply the pending log: one H2D copy of the rows and one K8 launch
        (the model on the CPU engine), then the DirectMap changes through
        the incremental K6 path.  An empty log costs nothing."""
        if self._mship_rows:
            rows, self._mship_rows = self._mship_rows, {}
            m64 = (1 << 64) - 1
            flat = []
            for r, (clear, set_, reset) in rows.items():
                flat += [r, 1 if reset else 0,
                         clear & m64, (clear >> 64) & m64, (clear >> 128) & m64, clear >> 192,
                         set_ & m64, (set_ >> 64) & m64, (set_ >> 128) & m64, set_ >> 192]
            recs = torch.from_numpy(
                np.array(flat, dtype=np.uint64).view(np.int64).reshape(len(rows), 10))
            try:
                if self.use_gpu_ops:
                    if self._ctl_ops is None:
                        from ..ops import get_gpu_ctl_ops

                        self._ctl_ops = get_gpu_ctl_ops()
                    self._ctl_ops.membership_apply(self.sub_bitmap, self.ring_wpos,
                                                   recs.to(self.device))
                else:
                    ref.membership_apply(self.sub_bitmap, self.ring_wpos, recs)
            except Exception:
                self._mship_rows = rows   # nothing applied: the rows stay pending
                raise
            if self.loss_accounting:
                # K8 reset these cursors: their demand goes with them
                reset = [r for r, row in rows.items()
                         if row[2] and 0 <= r < self.n_recipients]
                if reset:
                    self.demand[torch.tensor(reset, dtype=torch.int64).to(self.device)] = 0
        self.directs.flush()

    # ---------------------------- the hot tick ----------------------------

    def _origin_tensor(self, origin, M: int) -> torch.Tensor:
        """Per-message origin as an int32 [M] tensor on the engine device
        (0 = from a local user, 1 = from a peer broker; None = all zeros)."""
        if origin is None:
            return torch.zeros(M, dtype=torch.int32, device=self.device)
        if not isinstance(origin, torch.Tensor):
            origin = torch.tensor(list(origin), dtype=torch.int32)
        assert origin.numel() == M, "origin must have one entry per message"
        return origin.to(device=self.device, dtype=torch.int32,
                         non_blocking=self.is_cuda).contiguous()

    def ingest(self, batch: bytes, offsets: List[int],
               staging: Optional[torch.Tensor] = None, origin=None):
        """H2D-copy one batch of serialized messages. Returns device (buf, offsets).

        `origin` (int32 [M] tensor or list; 0 = local user, 1 = peer broker)
        is copied alongside: the return value is then (buf, offsets, origin)
        with the device origin tensor to hand to tick().

        `staging`: an HBM-pool slice (hbm_pool.PoolBytes.tensor) to land the
        batch in instead of a fresh allocation — the bounded/backpressured
        ingest path (reference limiter semantics).  Safe to reuse after the
        caller drops the allocation because all consumers are stream-ordered
        behind this copy on the engine's stream."""
        if origin is not None:
            buf, off = self.ingest(batch, offsets, staging)
            return buf, off, self._origin_tensor(origin, len(offsets) - 1)
        host = torch.frombuffer(bytearray(batch), dtype=torch.uint8)
        off = torch.tensor(offsets, dtype=torch.int64)
        if staging is not None:
            assert staging.numel() >= host.numel()
            dst = staging[:host.numel()]
            dst.copy_(host, non_blocking=self.is_cuda)
            if self.is_cuda:
                return dst, off.to(self.device, non_blocking=True)
            return dst, off
        if self.is_cuda:
            return host.to(self.device, non_blocking=True), off.to(self.device, non_blocking=True)
        return host, off

    def tick(self, buf: torch.Tensor, offsets: torch.Tensor,
             host_batch: Optional[bytes] = None,
             host_offsets: Optional[List[int]] = None,
             uniform_wire_len: Optional[int] = None,
             origin=None) -> TickStats:
        """Run the full pipeline on one ingested batch already on device.

        uniform_wire_len: if the caller knows every message in the batch has
        this exact wire length (and fanout_wire is set), the flat-index K3
        variant runs at ~100% lane utilization.

        origin: per-message int32 [M] tensor or list, 0 = from a local user,
        1 = from a peer broker (None = all local).  Remote-origin messages
        never reach a peer ring (single hop).

        With a ref_threshold, host_batch and host_offsets are required on
        both engines: a batch that holds a by-reference message is retained
        until the next drain."""
        self.flush_membership()
        ref_base = 0
        if self.ref_threshold is not None:
            if host_batch is None or host_offsets is None:
                raise ValueError("by-reference delivery needs host_batch and host_offsets")
            ref_base = self._retain_batch(host_batch, host_offsets)
        if self.use_gpu_ops:
            return self._tick_gpu(buf, offsets, uniform_wire_len, origin, ref_base)
        assert host_batch is not None and host_offsets is not None
        return self._tick_cpu(host_batch, host_offsets, origin, ref_base)

    def _retain_batch(self, host_batch, host_offsets) -> int:
        """Keep `host_batch` for the next drain if any of its messages goes
        by reference.  Returns the batch's offset in the reference buffer."""
        thr = self.ref_threshold
        base = self._ref_base
        if any(host_offsets[i + 1] - host_offsets[i] >= thr
               for i in range(len(host_offsets) - 1)):
            self._ref_batches.append(host_batch)
            self._ref_base = base + len(host_batch)
        return base

    def _discard_ref_batches(self) -> None:
        self._ref_batches = []
        self._ref_base = 0

    def _k2b_block_scratch(self, M: int):
        """Lazily (re)allocate the block-K2b scratch for batches up to M
        messages: [NB][W*64] counts + prefixes, per-user base/fit/dst."""
        NB = (M + 31) // 32
        W64 = self.W * 64
        cur = self._k2b_scratch
        if cur is not None and cur[0] >= NB:
            return cur[1]
        o32 = dict(dtype=torch.int32, device=self.device)
        bufs = (
            torch.empty(NB * W64, **o32),              # bcount
            torch.empty(NB * W64, **o32),              # pprefix
            torch.empty(W64, **o32),                   # ubase
            torch.empty(W64, **o32),                   # ufit
            torch.empty(W64, dtype=torch.int64, device=self.device),  # udst
        )
        self._k2b_scratch = (NB, bufs)
        return bufs

    def _assign_emit(self, ops, mask_t, payload_len, rec: int, M: int) -> None:
        """Dispatch K2b: block-parallel pipeline for uniform records (fills
        the chip at any population — the one-lane-per-user fused kernel
        runs only ~W waves), fused kernel otherwise."""
        if rec and self.use_gpu_ops:
            bcount, pprefix, ubase, ufit, udst = self._k2b_block_scratch(M)
            ops.assign_emit_blocks_t(
                mask_t, self.ring_wpos, self.ring_bytes, self.n_recipients,
                bcount, pprefix, ubase, ufit, udst,
                self._pairs, self._drops, self._n_pairs, rec,
            )
        else:
            ops.assign_emit_fused_t(
                mask_t, payload_len, self.ring_wpos, self.ring_bytes, self.n_recipients,
                self._pairs, self._drops, self._n_pairs, rec,
            )

    def _fused_tick_ok(self, uniform_wire_len: Optional[int], origin) -> bool:
        """The shape the fused native tick serves: uniform wire records that
        the flat fan-out takes, broadcast only, one broker, all inline.
        Never with loss accounting: the fused tick keeps its mask in LDS, so
        there is no mask_t for the demand kernel to read."""
        return (self.fused_tick and not self.loss_accounting
                and self.fanout_wire and uniform_wire_len is not None
                and not self.direct_enabled and self.n_peer_slots == 0
                and origin is None and self.ref_threshold is None
                and ring_rec(uniform_wire_len) <= self._flat_max_rec)

    def _tick_fused(self, buf: torch.Tensor, offsets: torch.Tensor,
                    uniform_wire_len: int, M: int) -> TickStats:
        ops = self._ops
        # engine-owned scratch, grown to the largest shape seen so far; a
        # shape that repeats needs no second look at its sizes
        shape = (M, self.W, uniform_wire_len)
        s64, s32 = self._fused_scratch or (None, None)
        if shape != self._fused_scratch_shape:
            n64, n32 = ops.uniform_tick_scratch_sizes(M, self.W, ring_rec(uniform_wire_len))
            if s64 is None or s64.numel() < n64 or s32.numel() < n32:
                s64 = torch.empty(max(n64, 0 if s64 is None else s64.numel()),
                                  dtype=torch.int64, device=self.device)
                s32 = torch.empty(max(n32, 0 if s32 is None else s32.numel()),
                                  dtype=torch.int32, device=self.device)
                self._fused_scratch = (s64, s32)
            self._fused_scratch_shape = shape
        seq_base = self.seq
        self.seq += M
        ops.tick_uniform_broadcast(
            buf, offsets, self.hash_seed, self.sub_bitmap, self.ring_wpos, self.ring_bytes,
            self.n_recipients, self._pairs, self._drops, self._n_pairs, self._n_sparse,
            s64, s32, uniform_wire_len, seq_base, self.egress,
            1 if self.nt_fanout else 0, 1 if self._dense_fanout else 0)
        self.fused_ticks += 1
        return TickStats(n_messages=M)

    def _tick_gpu(self, buf: torch.Tensor, offsets: torch.Tensor,
                  uniform_wire_len: Optional[int] = None, origin=None,
                  ref_base: int = 0) -> TickStats:
        ops = self._ops
        M = offsets.shape[0] - 1
        if M > 0 and self._fused_tick_ok(uniform_wire_len, origin):
            return self._tick_fused(buf, offsets, uniform_wire_len, M)
        disc, payload_off, payload_len, topics_off, topics_cnt, recip_hash, _ts = ops.parse_batch(
            buf, offsets, self.hash_seed
        )
        # peer plane: with peer slots or an explicit origin the origin-aware
        # K2a / K5b variants run; otherwise exactly the kernels of a lone
        # broker (topic_mask_t, emit_direct)
        peer_plane = self.n_peer_slots > 0 or origin is not None
        if peer_plane:
            origin = self._origin_tensor(origin, M)
            mask_t = ops.topic_mask_origin_t(self.sub_bitmap, buf, topics_off, topics_cnt,
                                             disc, origin, self.n_users)
        else:
            mask_t = ops.topic_mask_t(self.sub_bitmap, buf, topics_off, topics_cnt, disc)
        if self.fanout_wire:
            payload_off = offsets[:-1].contiguous()
            payload_len = (offsets[1:] - offsets[:-1]).to(torch.int32).contiguous()
        # fused sync-free pipeline on the transposed mask: one kernel counts
        # + claims slots atomically (wave-aggregated) + emits; the pair
        # count stays on device
        self._n_pairs.zero_()
        uniform = self.fanout_wire and uniform_wire_len is not None
        thr = self.ref_threshold
        # ring_len: what K2b / K5b claim ring space for — 0 (a bare header)
        # for a by-reference message.  A uniform length at or above the
        # threshold leaves the flat path: its records are headers only.
        ring_len = payload_len
        if thr is not None:
            if uniform and uniform_wire_len >= thr:
                uniform = False
            if not uniform:
                ring_len = torch.where(payload_len >= thr, 0, payload_len).to(torch.int32)
        rec = ring_rec(uniform_wire_len) if uniform else 0
        self._assign_emit(ops, mask_t, ring_len, rec, M)
        owner = None
        if self.direct_enabled:
            # K5 lookup + K5b on-device delivery-pair emission: direct pairs
            # append to the same pair list, all consumed by the single
            # fan-out below — no host sync anywhere in the tick.
            # (uniform_wire_len callers promise Direct messages share the
            # same padded wire length as broadcasts.)
            owner = ops.direct_lookup(self.direct_keys, self.direct_vals, recip_hash)
            if peer_plane:
                ops.emit_direct_peers(disc, owner, origin, payload_off, ring_len,
                                      self.ring_bytes, self.n_users, self.n_peer_slots,
                                      self.ring_wpos, self._n_pairs, self._pairs,
                                      self._drops)
            else:
                ops.emit_direct(disc, owner, payload_off, ring_len, self.ring_bytes,
                                self.ring_wpos, self._n_pairs, self._pairs, self._drops)
        if self._acct_ops is not None and M > 0:
            # K9: what this tick wanted to deliver, per recipient, from the
            # inputs K2b and K5b claimed from — one launch, nothing read back
            self._acct_ops.recipient_demand(
                self.demand, mask_t, ring_len.contiguous(), disc, owner,
                origin if peer_plane else None, self.n_users, self.n_peer_slots)
        seq_base = self.seq
        self.seq += M
        nt = 1 if self.nt_fanout else 0
        # flat (unit-per-lane) wins on small records where wave-per-pair
        # would idle lanes on the tail pass; at >=4 KiB records a wave's 64
        # passes are already ~fully utilized and flat's per-unit index math
        # costs ~3% (measured on the 64 KiB mixed bench) — use wave there.
        if uniform and rec <= self._flat_max_rec:
            units = rec // 16
            # uniform records: wire length passed as a scalar — saves the
            # per-unit payload_len load (~1 load per 16 B stored)
            ops.fanout_flat2(buf, payload_off, payload_len, self._pairs, seq_base,
                             self._n_pairs, units, self.egress, nt, 0,
                             uniform_wire_len)
        else:
            seq = torch.arange(seq_base, seq_base + M, dtype=torch.int32, device=self.device)
            if thr is not None:
                ops.fanout_ref(buf, payload_off, payload_len, self._pairs, seq,
                               self._n_pairs, self.egress, nt, 0, thr, ref_base)
            else:
                ops.fanout_wave(buf, payload_off, payload_len, self._pairs, seq,
                                self._n_pairs, self.egress, nt, 0)
        return TickStats(n_messages=M)

    def _graph_tick_body(self, buf: torch.Tensor, offsets: torch.Tensor, units: int) -> None:
        """The capturable broadcast-tick body (uniform wire records, no host
        syncs, no direct routing): parse -> mask -> fused emit -> flat3
        fan-out -> device seq bump.  All tensors fixed-address."""
        ops = self._ops
        M = offsets.shape[0] - 1
        disc, _po, _pl, topics_off, topics_cnt, _rh, _ts = ops.parse_batch(
            buf, offsets, self.hash_seed
        )
        mask_t = ops.topic_mask_t(self.sub_bitmap, buf, topics_off, topics_cnt, disc)
        payload_off = offsets[:-1].contiguous()
        payload_len = (offsets[1:] - offsets[:-1]).to(torch.int32).contiguous()
        self._n_pairs.zero_()
        rec = units * 16
        self._assign_emit(ops, mask_t, payload_len, rec, M)
        ops.fanout_flat3(buf, payload_off, payload_len, self._pairs, self._seq_dev,
                         self._n_pairs, units, self.egress,
                         1 if self.nt_fanout else 0, 0, (units - 1) * 16)
        ops.seq_advance(self._seq_dev, M)

    def tick_graphed(self, buf: torch.Tensor, offsets: torch.Tensor,
                     uniform_wire_len: int) -> None:
        """hipGraph-captured broadcast tick: captured once per fixed
        (buf, offsets) pair, replayed thereafter (one host call instead of
        ~8 kernel launches). Requires fanout_wire + uniform records +
        direct_enabled=False (the broadcast-bench shape)."""
        self.flush_membership()
        if self.loss_accounting:
            # the warm-up runs the body for real and the captured body has no
            # demand kernel: neither can be squared with the accounting
            raise ValueError("tick_graphed does not run with loss_accounting")
        assert self.fanout_wire and not self.direct_enabled
        if self.ref_threshold is not None and uniform_wire_len >= self.ref_threshold:
            raise ValueError("tick_graphed carries inline records only: "
                             f"wire length {uniform_wire_len} is at or above "
                             f"ref_threshold {self.ref_threshold}")
        units = ring_rec(uniform_wire_len) // 16
        key = (buf.data_ptr(), offsets.data_ptr(), units)
        g = self._graphs.get(key)
        if g is None:
            # warmup runs the body for real and mutates broker state —
            # snapshot and restore ring cursors / seq / drop counter
            saved = (self.ring_wpos.clone(), self._seq_dev.clone(), self._drops.clone())
            side = torch.cuda.Stream(device=self.device)
            side.wait_stream(torch.cuda.current_stream(self.device))
            with torch.cuda.stream(side):
                for _ in range(2):  # warmup (allocator + kernels)
                    self._graph_tick_body(buf, offsets, units)
            torch.cuda.current_stream(self.device).wait_stream(side)
            torch.cuda.synchronize(self.device)
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                self._graph_tick_body(buf, offsets, units)
            self.ring_wpos.copy_(saved[0])
            self._seq_dev.copy_(saved[1])
            self._drops.copy_(saved[2])
            self._graphs[key] = g
        g.replay()

    def _tick_cpu(self, batch: bytes, offsets: List[int], origin=None,
                  ref_base: int = 0) -> TickStats:
        pr = ref.parse_batch(batch, offsets, self.hash_seed)
        M = len(offsets) - 1
        origin = self._origin_tensor(origin, M)
        mask = ref.topic_mask_origin(self.sub_bitmap, batch, pr.topics_off, pr.topics_cnt,
                                     pr.disc, origin, self.n_users)
        if self.fanout_wire:
            pr.payload_off = torch.tensor(offsets[:-1], dtype=torch.int64)
            pr.payload_len = (
                torch.tensor(offsets[1:], dtype=torch.int64)
                - torch.tensor(offsets[:-1], dtype=torch.int64)
            ).to(torch.int32)
        thr = self.ref_threshold
        ring_len = pr.payload_len if thr is None else ref.ring_lengths(pr.payload_len, thr)
        owner = ref.direct_lookup(self.direct_keys, self.direct_vals, pr.recip_hash)
        if self.loss_accounting:
            ref.recipient_demand(mask, ring_len, pr.disc, owner, origin, self.n_users,
                                 self.n_peer_slots, self.demand)

        def fan(p_user, p_msg, p_dst):
            if thr is None:
                ref.fanout(batch, pr.payload_off, pr.payload_len, p_user, p_msg, p_dst,
                           seq, arr)
            else:
                ref.fanout_ref(batch, pr.payload_off, pr.payload_len, p_user, p_msg, p_dst,
                               seq, arr, thr, ref_base)

        pair_user, pair_msg, pair_dst, drops = ref.assign_emit(
            mask, ring_len, self.ring_wpos, self.ring_bytes, self.n_recipients
        )
        seq = torch.arange(self.seq, self.seq + M, dtype=torch.int32)
        self.seq += M
        arr = bytearray(self.egress.numpy().tobytes())  # copy-in; copied back below
        fan(pair_user, pair_msg, pair_dst)
        # Direct deliveries claim ring space after the broadcasts, in message
        # order: local users and, for local-origin messages, peer slots
        d_user, d_msg, d_dst, d_drops = ref.emit_direct_peers(
            pr.disc, owner, origin, ring_len, self.ring_wpos, self.ring_bytes,
            self.n_users, self.n_peer_slots)
        fan(d_user, d_msg, d_dst)
        self.egress.copy_(torch.frombuffer(arr, dtype=torch.uint8))
        return TickStats(n_messages=M, n_deliveries=int(pair_user.shape[0]),
                         n_drops=drops + d_drops)

    # ------------------------------- drain ---------------------------------

    def drain_cursors(self) -> torch.Tensor:
        """Read back ring cursors (the per-tick notify) and reset them.
        Retained by-reference batches are discarded: the cursors were the
        only way to reach the records that point into them."""
        self.flush_membership()
        self._discard_ref_batches()
        self._scan_losses()
        if self.fused_tick and self.use_gpu_ops and self.is_cuda:
            if self._drain_bufs is None:
                self._drain_bufs = (
                    torch.empty_like(self.ring_wpos),
                    torch.empty(self.ring_wpos.shape, dtype=torch.int64, pin_memory=True),
                )
            staging, host = self._drain_bufs
            self._ops.drain_cursors(self.ring_wpos, staging, host)  # synchronises
            self._collect_losses()
            return host.clone()
        wpos = self.ring_wpos.detach().clone().to("cpu")
        self.ring_wpos.zero_()
        self._collect_losses()
        return wpos

    def drain_compact(self) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
        """Zero-copy tick drain: K7 gathers every ring's used prefix into one
        contiguous device staging buffer, then ONE D2H lands it in pinned
        host memory — the per-user Python read_ring loop (one D2H + one
        interpreter round-trip per user) disappears.  Returns
        (wpos[N] cpu, offsets[N+1] cpu, staging host uint8) where user u's
        records occupy staging[offsets[u]:offsets[u+1]].  Reference analog:
        the Arc-clone fan-out never copies per recipient either
        (user/sender.rs:16-33).  Retained by-reference batches are discarded
        (use drain_compact_ref to get them)."""
        self.flush_membership()
        self._discard_ref_batches()
        return self._drain_compact()

    def drain_compact_ref(self):
        """drain_compact plus the reference buffer: returns (wpos, offsets,
        staging, refbuf).  A by-reference record's ref_off indexes refbuf:
        the retained host batch itself when the drain covers one (no copy),
        the retained batches joined in tick order otherwise, b"" when
        nothing went by reference.  Clears the retained batches."""
        self.flush_membership()
        batches = self._ref_batches
        self._discard_ref_batches()
        if len(batches) == 1:
            refbuf = batches[0]
        else:
            refbuf = b"".join(bytes(b) for b in batches)
        return (*self._drain_compact(), refbuf)

    def drain_framed(self):
        """drain_compact with the per-record work done on the device: returns
        (wpos, offsets, frame_len, frame_cnt, staging), all on the host.
        Recipient r's bytes are staging[offsets[r] : offsets[r] + frame_len[r]]:
        frame_cnt[r] frames [u32 big-endian len][message] back to back, in
        the order parse_ring_records gives, ready for the socket.
        frame_cnt[r] == -1 (only for an out-of-order ring of more than
        FRAME_SORT_MAX records, which a drain per tick never produces): the
        bytes are the raw ring prefix, frame_len[r] == wpos[r].  Not with
        ref_threshold: a by-reference record's body is in host memory."""
        if self.ref_threshold is not None:
            raise ValueError("drain_framed cannot frame by-reference records: "
                             "the engine was built with a ref_threshold")
        self.flush_membership()
        self._discard_ref_batches()
        return self._drain_compact(framed=True)

    def _drain_compact(self, framed: bool = False):
        """drain_compact's body; framed: drain_framed's, which differs in the
        kernel that fills the staging (K11 for K7) and in the two per-recipient
        arrays that come back with it."""
        R = self.n_recipients
        self._scan_losses()
        if not self.use_gpu_ops:
            wpos = self.ring_wpos.detach().clone()
            self.ring_wpos.zero_()
            offsets = torch.zeros(R + 1, dtype=torch.int64)
            torch.cumsum(wpos, 0, out=offsets[1:])
            total = int(offsets[-1])
            staging = torch.empty(total, dtype=torch.uint8)
            if framed:
                frame_len = torch.zeros(R, dtype=torch.int64)
                frame_cnt = torch.zeros(R, dtype=torch.int32)
                ref.frame_rings(self.egress, self.ring_bytes, wpos, offsets[:R], staging,
                                frame_len, frame_cnt)
                return wpos, offsets, frame_len, frame_cnt, staging
            for u in range(R):
                n = int(wpos[u])
                if n:
                    s = u * self.ring_bytes
                    staging[int(offsets[u]):int(offsets[u + 1])] = self.egress[s:s + n]
            return wpos, offsets, staging
        wpos_dev = self.ring_wpos  # read by K7 / K11 before the reset below
        wpos = wpos_dev.detach().to("cpu")  # sync: cursor readback
        self._collect_losses()
        offsets = torch.zeros(R + 1, dtype=torch.int64)
        torch.cumsum(wpos, 0, out=offsets[1:])
        total = int(offsets[-1])
        if total == 0:
            self.ring_wpos.zero_()
            empty = torch.empty(0, dtype=torch.uint8)
            if framed:
                return (wpos, offsets, torch.zeros(R, dtype=torch.int64),
                        torch.zeros(R, dtype=torch.int32), empty)
            return wpos, offsets, empty
        # DOUBLE-buffered host staging: the caller may still be writing the
        # previous drain's frames to sockets (pipelined drains) while this
        # tick compacts into the other buffer; callers must not reuse a
        # buffer until its drain completed (see service._drain_egress)
        idx = self.next_staging_index()
        self._staging_flip = idx ^ 1
        if self._staging_dev is None or self._staging_dev.numel() < total:
            cap = max(total, 1 << 22)
            self._staging_dev = torch.empty(cap, dtype=torch.uint8, device=self.device)
            self._staging_host = [
                torch.empty(cap, dtype=torch.uint8, pin_memory=self.is_cuda)
                for _ in range(2)
            ]
        dst_off = offsets[:R].to(self.device, non_blocking=True)
        if framed:
            meta = self._frame_rings(wpos_dev, dst_off, int(wpos.max()))
        else:
            max_chunks = (int(wpos.max()) + (64 << 10) - 1) // (64 << 10)
            self._ops.compact_rings(self.egress, self.ring_bytes, wpos_dev, dst_off,
                                    self._staging_dev, max_chunks)
        self.ring_wpos.zero_()  # stream-ordered after K7's / K11's reads
        host = self._staging_host[idx]
        if host.numel() < total:  # staging grew since this buffer was made
            host = self._staging_host[idx] = torch.empty(
                self._staging_dev.numel(), dtype=torch.uint8, pin_memory=self.is_cuda)
        host[:total].copy_(self._staging_dev[:total])  # sync D2H
        if framed:
            # the two small copies were queued ahead of the D2H above, whose
            # synchronise made them readable
            return wpos, offsets, meta[0].clone(), meta[1].clone(), host[:total]
        return wpos, offsets, host[:total]

    def _frame_rings(self, wpos_dev, dst_off, max_wpos: int):
        """K11 into the device staging, and frame_len / frame_cnt on their way
        to pinned host memory (not waited for).  Returns the two host tensors."""
        if self._drain_ops is None:
            from ..ops import get_gpu_drain_ops

            self._drain_ops = get_gpu_drain_ops()
        R = self.n_recipients
        if self._frame_meta is None:
            self._frame_meta = (
                torch.empty(R, dtype=torch.int64, device=self.device),
                torch.empty(R, dtype=torch.int32, device=self.device),
                torch.empty(R, dtype=torch.int64, pin_memory=self.is_cuda),
                torch.empty(R, dtype=torch.int32, pin_memory=self.is_cuda),
            )
        n_index = self._staging_dev.numel() // 16
        if self._frame_index is None or self._frame_index.shape[0] < n_index:
            self._frame_index = torch.empty((n_index, 4), dtype=torch.int32,
                                            device=self.device)
        len_dev, cnt_dev, len_host, cnt_host = self._frame_meta
        chunk = self._drain_ops.CHUNK_BYTES
        max_chunks = (min(max_wpos, self.ring_bytes) + chunk - 1) // chunk
        self._drain_ops.frame_rings(self.egress, self.ring_bytes, wpos_dev, dst_off,
                                    self._staging_dev, len_dev, cnt_dev, self._frame_index,
                                    max_chunks)
        len_host.copy_(len_dev, non_blocking=True)
        cnt_host.copy_(cnt_dev, non_blocking=True)
        return len_host, cnt_host

    # --------------------------- loss accounting ---------------------------

    def _scan_losses(self) -> None:
        """First step of every drain, before anything reads-and-resets the
        cursors.  GPU: K10 queues its list and a 4-byte count copy into pinned
        memory on the engine's stream and does not wait; the drain's own
        synchronise follows and _collect_losses() then reads the count.
        CPU: the model, merged at once."""
        if not self.loss_accounting:
            return
        if self._acct_ops is None:
            self._merge_losses(ref.loss_scan(self.demand, self.ring_wpos))
            return
        self._acct_ops.loss_scan(self.demand, self.ring_wpos, self._lossy, self._n_lossy,
                                 self._n_lossy_host)

    def _collect_losses(self) -> None:
        """After the drain's synchronise: the list is copied only when the
        scan found a lossy recipient (the rare path)."""
        if self._acct_ops is None:
            return
        n = int(self._n_lossy_host[0])
        if n:
            self._merge_losses(self._lossy[:n].to("cpu").tolist())

    def _merge_losses(self, rows) -> None:
        for r, d in rows:
            self._losses[r] = self._losses.get(r, 0) + d

    def take_losses(self) -> Dict[int, int]:
        """Recipient index -> ring bytes lost (demanded by the ticks, not
        delivered), as found by the drains since the previous call; clears
        the record.  Always empty without loss_accounting."""
        losses, self._losses = self._losses, {}
        return losses

    def next_staging_index(self) -> int:
        """Which host staging buffer the NEXT drain_compact or drain_framed
        will fill."""
        return self._staging_flip

    def read_ring(self, user_idx: int, nbytes: Optional[int] = None) -> bytes:
        n = self.ring_bytes if nbytes is None else nbytes
        start = user_idx * self.ring_bytes
        return bytes(self.egress[start : start + n].to("cpu").numpy().tobytes())

