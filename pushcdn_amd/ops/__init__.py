"""Kernel op access.

``get_gpu_ops()`` returns the compiled CDNA4 extension.  On a machine with a
GPU a missing/unbuildable extension is a **hard error** — there is no silent
eager fallback on the GPU path.  On CPU-only machines tests use
``pushcdn_amd.ops.reference`` instead.
"""

from __future__ import annotations

_gpu_mod = None


def get_gpu_ops():
    global _gpu_mod
    if _gpu_mod is not None:
        return _gpu_mod
    from .build import BUILD_DIR, build_gpu, load_gpu_prebuilt

    import torch

    so = BUILD_DIR / "pushcdn_gpu.so"
    if so.exists():
        try:
            _gpu_mod = load_gpu_prebuilt()
            return _gpu_mod
        except ImportError:
            pass
    if torch.cuda.is_available():
        # On a GPU box the extension must have been built (it travels with
        # the snapshot). Rebuilding silently could mask a stale-binary bug —
        # but a from-source build is still better than not running at all.
        _gpu_mod = build_gpu()
        return _gpu_mod
    _gpu_mod = build_gpu()
    return _gpu_mod


_gpu_ctl_mod = None


def get_gpu_ctl_ops():
    """The device-state maintenance extension (``pushcdn_gpu_ctl``: K8
    membership_apply), under the same rule as ``get_gpu_ops()``."""
    global _gpu_ctl_mod
    if _gpu_ctl_mod is not None:
        return _gpu_ctl_mod
    from .build import GPU_CTL_BUILD_DIR, build_gpu_ctl, load_gpu_ctl_prebuilt

    if (GPU_CTL_BUILD_DIR / "pushcdn_gpu_ctl.so").exists():
        try:
            _gpu_ctl_mod = load_gpu_ctl_prebuilt()
            return _gpu_ctl_mod
        except ImportError:
            pass
    _gpu_ctl_mod = build_gpu_ctl()
    return _gpu_ctl_mod


_gpu_acct_mod = None


def get_gpu_acct_ops():
    """The loss-accounting extension (``pushcdn_gpu_acct``: K9
    recipient_demand, K10 loss_scan), under the same rule as
    ``get_gpu_ops()``."""
    global _gpu_acct_mod
    if _gpu_acct_mod is not None:
        return _gpu_acct_mod
    from .build import GPU_ACCT_BUILD_DIR, build_gpu_acct, load_gpu_acct_prebuilt

    if (GPU_ACCT_BUILD_DIR / "pushcdn_gpu_acct.so").exists():
        try:
            _gpu_acct_mod = load_gpu_acct_prebuilt()
            return _gpu_acct_mod
        except ImportError:
            pass
    _gpu_acct_mod = build_gpu_acct()
    return _gpu_acct_mod


_gpu_drain_mod = None


def get_gpu_drain_ops():
    """The framed-drain extension (``pushcdn_gpu_drain``: K11 frame_rings),
    under the same rule as ``get_gpu_ops()``."""
    global _gpu_drain_mod
    if _gpu_drain_mod is not None:
        return _gpu_drain_mod
    from .build import GPU_DRAIN_BUILD_DIR, build_gpu_drain, load_gpu_drain_prebuilt

    if (GPU_DRAIN_BUILD_DIR / "pushcdn_gpu_drain.so").exists():
        try:
            _gpu_drain_mod = load_gpu_drain_prebuilt()
            return _gpu_drain_mod
        except ImportError:
            pass
    _gpu_drain_mod = build_gpu_drain()
    return _gpu_drain_mod
