"""In-tree build of the HIP/C++ extensions.

Five modules:
  - ``pushcdn_gpu``  — CDNA4 data-plane kernels (csrc/hip/*.hip) + torch bindings,
                       compiled for gfx950 only.
  - ``pushcdn_gpu_ctl`` — device-state maintenance kernels
                       (csrc/hip/membership.hip) + torch bindings, gfx950 only.
  - ``pushcdn_gpu_acct`` — per-recipient loss-accounting kernels
                       (csrc/hip/accounting.hip) + torch bindings, gfx950 only.
  - ``pushcdn_gpu_drain`` — the framed-drain kernels
                       (csrc/hip/framed_drain.hip) + torch bindings, gfx950 only.
  - ``pushcdn_core`` — host C++ (wire serde, BLS-over-BN254, CRDT) via pybind11.

Everything builds into ``<repo>/build/`` (in-tree, so the .so files travel to
the GPU box with the snapshot).  ``__graft_entry__.build()`` calls
``build_all()``; at import time we only *load* what exists, and on a GPU
machine a missing GPU extension is a hard error (no silent eager fallback).
"""

from __future__ import annotations

import os
import sys
from pathlib import Path

REPO_ROOT = Path(__file__).resolve().parent.parent.parent
CSRC = REPO_ROOT / "csrc"
BUILD_DIR = REPO_ROOT / "build"

GPU_SOURCES = [
    CSRC / "gpu_bindings.cpp",
    CSRC / "hip" / "dataplane.hip",
    CSRC / "hip" / "bls_kernels.hip",
]

# Built in a directory of its own: the extension builder keeps one
# build.ninja per build directory.
GPU_CTL_BUILD_DIR = BUILD_DIR / "ctl"
GPU_CTL_SOURCES = [
    CSRC / "gpu_ctl_bindings.cpp",
    CSRC / "hip" / "membership.hip",
]

# Likewise a directory of its own.
GPU_ACCT_BUILD_DIR = BUILD_DIR / "acct"
GPU_ACCT_SOURCES = [
    CSRC / "gpu_acct_bindings.cpp",
    CSRC / "hip" / "accounting.hip",
]

# And the framed drain's.
GPU_DRAIN_BUILD_DIR = BUILD_DIR / "drain"
GPU_DRAIN_SOURCES = [
    CSRC / "gpu_drain_bindings.cpp",
    CSRC / "hip" / "framed_drain.hip",
]

os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")


def _build_torch_ext(name: str, srcs, build_dir: Path, verbose: bool):
    from torch.utils.cpp_extension import load

    build_dir.mkdir(parents=True, exist_ok=True)
    sources = [str(s) for s in srcs if s.exists()]
    # ninja's rules for hipcc lack header depfiles: if any shared header is
    # newer than a built object, touch the sources so the rebuild triggers.
    headers = list(CSRC.glob("*.h")) \
        + list((CSRC / "common").glob("*.h")) + list((CSRC / "bls").glob("*.h")) \
        + list((CSRC / "wire").glob("*.h")) + list((CSRC / "hip").glob("*.h"))
    if headers:
        newest_h = max(h.stat().st_mtime for h in headers)
        for src in srcs:
            if src.exists() and src.stat().st_mtime < newest_h:
                os.utime(src)
    mod = load(
        name=name,
        sources=sources,
        build_directory=str(build_dir),
        extra_cflags=["-O3", "-std=c++17"],
        extra_cuda_cflags=["-O3", "-std=c++17"],
        verbose=verbose,
    )
    return mod


def _load_prebuilt(name: str, so: Path):
    if not so.exists():
        raise ImportError(
            f"{name} extension not built (expected {so}); "
            "run __graft_entry__.build() first"
        )
    import importlib.util

    spec = importlib.util.spec_from_file_location(name, so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules[name] = mod
    return mod


def build_gpu(verbose: bool = False):
    """Compile (if needed) and load the GPU extension. Returns the module."""
    return _build_torch_ext("pushcdn_gpu", GPU_SOURCES, BUILD_DIR, verbose)


def load_gpu_prebuilt():
    """Load the already-built GPU extension without invoking the builder.

    Used on GPU boxes where the .so traveled with the snapshot; avoids any
    silent rebuild (and fails loudly if the extension is missing).
    """
    return _load_prebuilt("pushcdn_gpu", BUILD_DIR / "pushcdn_gpu.so")


def build_gpu_ctl(verbose: bool = False):
    """Compile (if needed) and load the device-state maintenance extension
    (K8 membership_apply). Returns the module."""
    return _build_torch_ext("pushcdn_gpu_ctl", GPU_CTL_SOURCES, GPU_CTL_BUILD_DIR, verbose)


def load_gpu_ctl_prebuilt():
    """load_gpu_prebuilt for the maintenance extension."""
    return _load_prebuilt("pushcdn_gpu_ctl", GPU_CTL_BUILD_DIR / "pushcdn_gpu_ctl.so")


def build_gpu_acct(verbose: bool = False):
    """Compile (if needed) and load the loss-accounting extension
    (K9 recipient_demand, K10 loss_scan). Returns the module."""
    return _build_torch_ext("pushcdn_gpu_acct", GPU_ACCT_SOURCES, GPU_ACCT_BUILD_DIR, verbose)


def load_gpu_acct_prebuilt():
    """load_gpu_prebuilt for the loss-accounting extension."""
    return _load_prebuilt("pushcdn_gpu_acct", GPU_ACCT_BUILD_DIR / "pushcdn_gpu_acct.so")


def build_gpu_drain(verbose: bool = False):
    """Compile (if needed) and load the framed-drain extension
    (K11 frame_rings). Returns the module."""
    return _build_torch_ext("pushcdn_gpu_drain", GPU_DRAIN_SOURCES, GPU_DRAIN_BUILD_DIR, verbose)


def load_gpu_drain_prebuilt():
    """load_gpu_prebuilt for the framed-drain extension."""
    return _load_prebuilt("pushcdn_gpu_drain", GPU_DRAIN_BUILD_DIR / "pushcdn_gpu_drain.so")


CORE_SOURCES = [CSRC / "core_bindings.cpp"]


def build_core(verbose: bool = False):
    """Compile (if needed) and load the host C++ core (pybind11, no torch)."""
    import importlib.util
    import pybind11
    import subprocess
    import sysconfig

    BUILD_DIR.mkdir(exist_ok=True)
    so = BUILD_DIR / "pushcdn_core.so"
    srcs = [str(s) for s in CORE_SOURCES]
    deps = (list((CSRC / "common").glob("*.h")) + list((CSRC / "bls").glob("*.h"))
            + list((CSRC / "wire").glob("*.h")) + list((CSRC / "state").glob("*.h"))
            + list((CSRC / "net").glob("*.h")) + CORE_SOURCES)
    newest_dep = max(p.stat().st_mtime for p in deps)
    if not so.exists() or so.stat().st_mtime < newest_dep:
        cmd = [
            "g++", "-O3", "-std=c++17", "-shared", "-fPIC",
            f"-I{pybind11.get_include()}",
            f"-I{sysconfig.get_paths()['include']}",
            f"-I{CSRC}",
            *srcs,
            "-o", str(so),
        ]
        if verbose:
            print(" ".join(cmd))
        subprocess.run(cmd, check=True)
    spec = importlib.util.spec_from_file_location("pushcdn_core", so)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    sys.modules["pushcdn_core"] = mod
    return mod
