"""MeshBroker — the GPU broker with its broker-plane on RCCL over xGMI.

One process per GPU (torchrun); the broker↔broker transport is the
RcclMesh collective exchange instead of framed TCP connections: each tick,
every broker contributes its ingest batch (wire bytes + offsets packed into
a fixed-capacity buffer) and receives every peer's batch over the
all-gather, then routes ALL batches through the local kernel pipeline —
remote batches deliver to local subscribers only, which is exactly the
reference's single-hop to_users_only semantics
(broker/handler.rs:151-161).

The user plane (TCP/TLS/memory transports, auth, permits) is unchanged from
the base Broker; the framed broker-mesh tasks (dialing, sync blasts) are
disabled — the communicator IS the mesh, and every broker sees every
message, so topic-interest sync is unnecessary for routing correctness
(exchange_p2p + interest maps are the bandwidth optimization for sparse
topologies).

Batch wire layout (what travels over the collective):
    [i64 n_messages][i64 offsets[n+1]  (absolute byte offsets)]
    [pad to 16-byte boundary][message bytes, each start 16-aligned]
"""

from __future__ import annotations

import asyncio
from typing import List, Optional, Tuple

import torch

from ..parallel.mesh import RcclMesh
from ..proto.limiter import Bytes
from .service import Broker, BrokerConfig


def pack_mesh_batch(msgs: List[bytes], capacity: int) -> Tuple[torch.Tensor, int, int]:
    """Pack wire messages into the travel layout. Returns
    (host uint8 tensor of `capacity`, n_messages, used_bytes)."""
    n = len(msgs)
    header_words = n + 2  # n + offsets[n+1]
    base = (header_words * 8 + 15) & ~15
    offsets = [base]
    total = base
    for raw in msgs:
        total += (len(raw) + 15) & ~15
        offsets.append(total)
    if total > capacity:
        raise ValueError(f"mesh batch overflow: {total} > {capacity}")
    buf = torch.zeros(capacity, dtype=torch.uint8)
    header = torch.tensor([n] + offsets, dtype=torch.int64)
    buf[: header_words * 8] = header.view(torch.uint8)
    pos = base
    for raw in msgs:
        if raw:  # torch.frombuffer rejects empty buffers
            buf[pos : pos + len(raw)] = torch.frombuffer(bytearray(raw), dtype=torch.uint8)
        pos += (len(raw) + 15) & ~15
    return buf, n, total


def unpack_mesh_offsets(view: torch.Tensor, n_messages: int) -> torch.Tensor:
    """Device (or host) int64 offsets tensor [n+1] out of a packed batch."""
    header_words = n_messages + 2
    return view[: header_words * 8].view(torch.int64)[1 : n_messages + 2].contiguous()


class MeshBroker(Broker):
    # C++ blob ingest is supported: the tick normalizes blob items into
    # per-message views for the collective pack
    BLOB_INGEST = True
    # the broker plane is the collective: no device peer rings here
    PEER_FORWARD = False
    # the collective tick delivers inline records only
    REF_DELIVERY = False
    # the collective tick has its own drain: no loss accounting here, so
    # config.gpu_overflow_policy has no effect
    OVERFLOW_POLICY = False
    # and it dispatches drain_compact's ring records itself, so
    # config.gpu_framed_drain has no effect
    FRAMED_DRAIN = False

    def __init__(self, config: BrokerConfig, batch_capacity: int = 1 << 22,
                 interest_routed: Optional[bool] = None) -> None:
        assert config.data_plane == "gpu", "MeshBroker is the GPU data-plane broker"
        super().__init__(config)
        self.batch_capacity = batch_capacity
        # interest_routed: ship batches only to peers whose subscribers
        # intersect the batch's topics, or whose owned-user digest
        # intersects the batch's direct-recipient digest (grouped P2P on
        # the xGMI links), instead of the all-gather.  Default: ON whenever
        # there are real peers (the reference also fans out per interested
        # broker, handler.rs:262-265).
        if interest_routed is None:
            import os

            interest_routed = int(os.environ.get("WORLD_SIZE", "1")) > 1
        self.interest_routed = interest_routed
        self.mesh: Optional[RcclMesh] = None
        self._carry: List[Bytes] = []  # messages that didn't fit last tick
        # per-phase wall-clock accumulators (seconds) — makes a SCALE run
        # diagnosable: pack/h2d/exchange/tick/drain medians per tick
        self.mesh_timings = {"pack": 0.0, "h2d": 0.0, "exchange": 0.0,
                             "tick": 0.0, "drain": 0.0, "ticks": 0}
        self._rebuild_task = None
        self._mesh_pause_until = 0.0  # test hook: simulated crash window
        # The collective exchange + kernel ticks run on ONE dedicated thread
        # so the asyncio loop keeps serving user IO / heartbeats while this
        # rank waits for its peers to align on the collective.  A single
        # worker also guarantees the communicator is never entered
        # concurrently (NCCL/gloo requirement).
        import concurrent.futures

        self._mesh_executor = concurrent.futures.ThreadPoolExecutor(
            max_workers=1, thread_name_prefix="mesh-tick")

    async def close(self) -> None:
        if self._rebuild_task is not None:
            self._rebuild_task.cancel()
        await super().close()
        self._mesh_executor.shutdown(wait=False, cancel_futures=True)

    # the framed broker mesh is replaced by the collective: no dialing, no
    # framed sync blasts; heartbeats still publish load for the marshal
    async def _heartbeat_task(self) -> None:
        while True:
            try:
                await self.discovery.perform_heartbeat(len(self.connections.users), 60.0)
            except Exception:
                pass
            await asyncio.sleep(self.config.heartbeat_interval_s)

    async def _sync_task(self) -> None:
        while True:  # nothing to sync: every broker sees every message
            await asyncio.sleep(3600)

    async def _send_partial_syncs(self) -> None:
        pass

    def _blocking_mesh_tick(self, msgs, dev_buf: Optional[torch.Tensor],
                            interests: int, owned_bits: int,
                            batch_topics: int, direct_bits: int):
        """One mesh tick's blocking half (runs on the dedicated mesh thread):
        pack, H2D, collective exchange, kernel tick per received batch,
        compacted drain.  Returns drain_compact's (wpos, offsets, staging).

        Peer failure (collective timeout/abort) tears the communicator down
        and the tick degrades to LOCAL-ONLY routing — the asyncio side then
        forwards batches to peers over framed TCP and runs the rebuild loop
        (reference semantics: evict the dead peer, keep serving,
        re-establish on heartbeat — heartbeat.rs:67-105)."""
        import time as _time

        tm = self.mesh_timings
        t0 = _time.perf_counter()
        host_buf, n_local, used_bytes = pack_mesh_batch(msgs, self.batch_capacity)
        t1 = _time.perf_counter()
        tm["pack"] += t1 - t0
        if dev_buf is not None:
            dev_buf.copy_(host_buf, non_blocking=True)
            send_buf = dev_buf
        else:
            send_buf = host_buf
        t2 = _time.perf_counter()
        tm["h2d"] += t2 - t1
        degraded = not self.mesh.healthy or _time.monotonic() < self._mesh_pause_until
        if degraded:
            if self.mesh.healthy:
                # simulated-crash window (test hook): stop participating
                self.mesh.teardown()
            exchanged = [(self.mesh.rank, send_buf, n_local, used_bytes)]
        else:
            try:
                if self.interest_routed:
                    exchanged = self.mesh.exchange_interest(
                        send_buf, n_local, used_bytes, batch_topics, interests,
                        direct_bits=direct_bits, owned_bits=owned_bits,
                    )
                else:
                    exchanged = self.mesh.exchange(send_buf, n_local, 0)
            except Exception:
                # peer failure: tear down, serve local-only; the asyncio
                # side starts TCP fallback + the rebuild loop
                self.mesh.teardown()
                exchanged = [(self.mesh.rank, send_buf, n_local, used_bytes)]
        t3 = _time.perf_counter()
        tm["exchange"] += t3 - t2
        for rank, view, n_msgs, _nbytes in exchanged:
            if n_msgs == 0:
                continue
            offsets = unpack_mesh_offsets(view, n_msgs)
            if self._engine.use_gpu_ops:
                self._engine.tick(view, offsets)
            else:
                host_bytes = bytes(view.numpy().tobytes())
                self._engine.tick(
                    view, offsets,
                    host_batch=host_bytes,
                    host_offsets=[int(x) for x in offsets],
                )
        t4 = _time.perf_counter()
        tm["tick"] += t4 - t3
        out = self._engine.drain_compact()
        tm["drain"] += _time.perf_counter() - t4
        tm["ticks"] += 1
        return out

    def _mesh_pause(self, seconds: float) -> None:
        """Test hook: simulate this broker crashing out of the mesh for
        `seconds` (stops participating in collectives, tears the
        communicator down), then rejoining via the rebuild rendezvous."""
        import time as _time

        self._mesh_pause_until = _time.monotonic() + seconds

    async def _mesh_rebuild_loop(self) -> None:
        """Re-establish the communicator after a peer failure.  Runs rebuild
        attempts on a DEDICATED thread (degraded ticks keep flowing on the
        mesh thread — they no longer touch the communicator) until every
        rank meets at the rendezvous store.  Meanwhile degraded ticks
        deliver locally and _forward_degraded ships batches to peers over
        framed TCP — the reference's keep-serving-while-reconnecting
        behavior."""
        import concurrent.futures
        import time as _time

        ex = concurrent.futures.ThreadPoolExecutor(
            max_workers=1, thread_name_prefix="mesh-rebuild")
        loop = asyncio.get_running_loop()
        try:
            while not self._closed:
                if _time.monotonic() < self._mesh_pause_until:
                    await asyncio.sleep(0.05)
                    continue
                ok = await loop.run_in_executor(
                    ex, self.mesh.rebuild, self.config.mesh_rebuild_timeout_s)
                if ok:
                    from ..utils.log import log

                    log.info("mesh communicator rebuilt (world=%d)",
                             self.mesh.world_size)
                    return
                await asyncio.sleep(0.2)
        finally:
            ex.shutdown(wait=False)
            self._rebuild_task = None

    async def _maybe_dial_peers(self) -> None:
        """While degraded, keep framed-TCP links to every live peer dialed
        (throttled; the inherited broker plane is still listening)."""
        import time as _time

        now = _time.monotonic()
        if now - getattr(self, "_last_dial_check", 0.0) < 0.3:
            return
        self._last_dial_check = now
        try:
            others = await self.discovery.get_other_brokers()
        except Exception:
            others = set()
        for peer in others:
            if peer not in self.connections.brokers:
                asyncio.get_running_loop().create_task(self._dial_broker(peer))

    async def _forward_degraded(self, entries) -> None:
        """Host-TCP fallback while the communicator is down: forward every
        queued message to the dialed peers; the receiving broker delivers
        with to_users_only/to_user_only semantics via its host plane —
        exactly the reference mesh path (broker/handler.rs:148-161)."""
        if self.connections.brokers:
            for data, _owner, _fwd in entries:
                await self.try_send_to_brokers(Bytes(bytes(data)))

    async def _gpu_tick_task(self) -> None:
        """Fixed-cadence mesh tick: pack queued local messages (possibly
        zero), exchange with every peer, route every rank's batch locally,
        drain egress back to user connections."""
        self.mesh = RcclMesh(self._engine.device, self.batch_capacity,
                             timeout_s=self.config.mesh_timeout_s)
        dev_buf = (
            torch.zeros(self.batch_capacity, dtype=torch.uint8, device=self._engine.device)
            if self._engine.is_cuda
            else None
        )
        from ..proto import message as msglib
        from ..utils.keyhash import fnv1a64

        while True:
            # collect up to a capacity-bounded batch; an oversize tick must
            # NEVER raise here — that would stall every peer's collective.
            # Queue items are either (Bytes, fwd) pairs or C++ ingest blobs
            # ("blob", bytes, end_offsets, fwds); both normalize to
            # (data_view, owner_or_None, fwd) entries.
            entries = self._carry
            self._carry = []
            used = sum((len(e[0]) + 15) & ~15 for e in entries)
            budget = self.batch_capacity - 16 * 4096  # header headroom
            overflow = False
            while not overflow and not self._gpu_queue.empty() and len(entries) < 4096:
                item = self._gpu_queue.get_nowait()
                if item[0] == "blob":
                    _tag, blob, ends, fwds = item
                    fs = 0
                    for i, fe in enumerate(ends):
                        view = memoryview(blob)[fs:fe]
                        fs = fe
                        padded = (len(view) + 15) & ~15
                        if used + padded > budget:
                            self._carry.append((view, None, fwds[i]))
                            overflow = True
                            continue  # keep normalizing the rest into carry
                        if overflow:
                            self._carry.append((view, None, fwds[i]))
                        else:
                            entries.append((view, None, fwds[i]))
                            used += padded
                else:
                    raw, fwd = item
                    padded = (len(raw.data) + 15) & ~15
                    if used + padded > budget:
                        self._carry.append((raw.data, raw, fwd))
                        overflow = True
                    else:
                        entries.append((raw.data, raw, fwd))
                        used += padded
            msgs = [e[0] for e in entries]
            # digest inputs come from loop-owned state (connections maps),
            # so compute them HERE; the exchange + ticks then run off-loop
            interests = owned_bits = batch_topics = direct_bits = 0
            if self.interest_routed:
                for t in self.connections.user_topics.get_values():
                    interests |= 1 << (t & 0xFF)
                # 64b digest of the direct users owned (connected) here —
                # the mesh-plane analog of the reference's DirectMap
                for pubkey in self._gpu_user_by_slot.values():
                    owned_bits |= 1 << (fnv1a64(pubkey, self._engine.hash_seed) & 63)
                # this batch's topic bitmap + direct-recipient digest come
                # from the ingest classification (frame-relative ranges);
                # items without fwd info (degraded-TCP arrivals) parse here
                for data, _owner, fwd in entries:
                    if fwd is None:
                        try:
                            r = msglib.parse_offsets(bytes(data))
                        except Exception:
                            continue
                        if r["disc"] == 4:
                            for t in data[r["topics_off"]:r["topics_off"] + r["topics_cnt"]]:
                                batch_topics |= 1 << t
                        elif r["disc"] == 3:
                            direct_bits |= 1 << (
                                fnv1a64(r["recipient"], self._engine.hash_seed) & 63)
                    else:
                        # ("b"/"d", value_bytes) from the asyncio receive
                        # loop, or ("b"/"d", start, end) frame-relative
                        # ranges from the C++ ingest classification
                        if len(fwd) == 2:
                            kind, val = fwd
                        else:
                            kind, fo, fe = fwd
                            val = bytes(data[fo:fe])
                        if kind == "b":
                            for t in val:
                                batch_topics |= 1 << t
                        else:
                            direct_bits |= 1 << (
                                fnv1a64(val, self._engine.hash_seed) & 63)
            wpos, offsets, staging = await asyncio.get_running_loop().run_in_executor(
                self._mesh_executor, self._blocking_mesh_tick,
                msgs, dev_buf, interests, owned_bits, batch_topics, direct_bits)
            await self._dispatch_egress(wpos, offsets, staging)
            if self.mesh.enabled and not self.mesh.healthy:
                await self._maybe_dial_peers()
                if entries:
                    await self._forward_degraded(entries)
                if self._rebuild_task is None:
                    self._rebuild_task = asyncio.get_running_loop().create_task(
                        self._mesh_rebuild_loop())
            for _data, owner, _fwd in entries:
                if owner is not None:
                    owner.drop()
            await asyncio.sleep(self.config.gpu_tick_interval_s)
