"""K11 on the GPU: the op against the hand-built cases (exact bytes, with the
sentinel intact outside every region), and the GPU engine's drain_framed
against the CPU engine's on the engine scenarios."""

import pytest
import torch

from tests import framed_drain_cases as fc

pytestmark = pytest.mark.gpu

CASES = {c.name: c for c in fc.all_cases()}


@pytest.fixture(scope="module")
def ops():
    from pushcdn_amd.ops import get_gpu_drain_ops

    return get_gpu_drain_ops()


def test_the_module_exports_the_cap(ops):
    from pushcdn_amd.ops.ring_format import FRAME_SORT_MAX

    assert ops.FRAME_SORT_MAX == FRAME_SORT_MAX >= 4096


@pytest.mark.parametrize("max_chunks", ["exact", "default"])
@pytest.mark.parametrize("name", CASES)
def test_op_matches_the_cases(ops, name, max_chunks):
    case = CASES[name]
    egress, wpos, dst_off, staging, frame_len, frame_cnt = fc.build_inputs(case, "cuda")
    index = torch.full((staging.numel() // 16, 4), -1, dtype=torch.int32, device="cuda")
    before = wpos.clone()
    args = (egress, case.ring_bytes, wpos, dst_off, staging, frame_len, frame_cnt, index)
    if max_chunks == "exact":
        used = min(int(wpos.max()), case.ring_bytes)
        ops.frame_rings(*args, (used + ops.CHUNK_BYTES - 1) // ops.CHUNK_BYTES)
    else:
        ops.frame_rings(*args)
    torch.cuda.synchronize()
    fc.check_outputs(case, dst_off.cpu(), staging.cpu(), frame_len.cpu(), frame_cnt.cpu())
    assert torch.equal(wpos, before)


def test_a_region_outside_the_staging_is_left_alone(ops):
    case = fc.Case("outside", 2048, fc.alignment_rings())
    egress, wpos, dst_off, staging, frame_len, frame_cnt = fc.build_inputs(case, "cuda")
    index = torch.zeros((staging.numel() // 16, 4), dtype=torch.int32, device="cuda")
    dst_off[1] = staging.numel() - int(wpos[1]) + 1          # one byte too far
    ops.frame_rings(egress, case.ring_bytes, wpos, dst_off, staging, frame_len, frame_cnt, index)
    torch.cuda.synchronize()
    assert frame_len.tolist()[1] == 0 and frame_cnt.tolist()[1] == 0
    only = fc.Case("outside", 2048, [case.rings[0], fc.EMPTY])
    fc.check_outputs(only, dst_off.cpu(), staging.cpu(), frame_len.cpu(), frame_cnt.cpu())


@pytest.mark.parametrize("kw", [
    {}, {"join": True}, {"burst": True},
    {"loss_accounting": True, "ring_bytes": 1024},
], ids=["plain", "join", "burst", "lossy"])
def test_gpu_engine_matches_cpu_engine(kw):
    eng, wpos, per, losses = fc.run_scenario("cuda:0", True, **kw)
    _cpu, wpos_c, per_c, losses_c = fc.run_scenario("cpu", True, **kw)
    assert wpos == wpos_c
    assert per == per_c
    assert losses == losses_c
    assert int(eng.ring_wpos.sum()) == 0
    w, _off, frame_len, frame_cnt, staging = eng.drain_framed()
    assert int(w.sum()) == 0 and int(frame_len.sum()) == 0 and int(frame_cnt.sum()) == 0
    assert staging.numel() == 0


def test_staging_buffers_flip_like_drain_compact():
    eng = fc.make_engine("cuda:0")
    eng.subscribe(0, [5])
    seen = []
    for _ in range(3):
        fc._tick(eng, fc.mixed_tick(0))
        seen.append(eng.next_staging_index())
        *_rest, staging = eng.drain_framed()
        assert staging.numel() > 0
    assert seen == [0, 1, 0]
