"""In-tree build of the HIP extension for gfx950.

The .so lands in dllama_amd/ops/_build/ (inside the repo) so it travels to
the GPU box with the snapshot — a JIT cache under ~/.cache would not.
Run `python -m dllama_amd.ops.build` or __graft_entry__.build().
"""

from __future__ import annotations

import os

_EXT_NAME = "dllama_hip"

# one translation unit per kernel family (plus host-only code and the pybind
# module), all sharing csrc/dllama_common.h. Named explicitly: hipify drops a
# <name>_hip.hip copy beside every source, which a csrc/*.hip glob would
# pick up on the second build.
_SOURCES = ("quant_norm.hip", "gemv.hip", "gemm.hip", "attn.hip", "moe.hip",
            "sync.hip", "sampler.hip", "logprob.hip", "host.hip", "module.hip")
_HEADER = "dllama_common.h"


def _sources():
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc")
    return [os.path.join(csrc, f) for f in _SOURCES]


def _paths():
    """(newest source file, build directory): callers compare the built
    library's mtime with the first, so it is the most recently modified of
    the sources and their shared header."""
    srcs = _sources()
    files = srcs + [os.path.join(os.path.dirname(srcs[0]), _HEADER)]
    here = os.path.dirname(os.path.abspath(__file__))
    return max(files, key=os.path.getmtime), os.path.join(here, "_build")


def _drop_objects_older_than_header(build_dir):
    """The ninja rule torch writes for hipcc records no header dependencies,
    so an edit to the shared header alone would recompile nothing: remove
    the objects that predate it and let ninja rebuild them."""
    header = os.path.join(os.path.dirname(_sources()[0]), _HEADER)
    for name in os.listdir(build_dir):
        obj = os.path.join(build_dir, name)
        if name.endswith(".o") and os.path.getmtime(obj) < os.path.getmtime(header):
            os.remove(obj)


def load_extension(verbose: bool = False):
    os.environ.setdefault("PYTORCH_ROCM_ARCH", "gfx950")
    os.environ.setdefault("MAX_JOBS", "8")
    from torch.utils.cpp_extension import load
    _, build_dir = _paths()
    os.makedirs(build_dir, exist_ok=True)
    _drop_objects_older_than_header(build_dir)
    # -mavx2/-mfma vectorize the HOST-side CPU Q40 matmul (hipcc applies
    # x86 flags to the host pass only); AVX2 is safe on every EPYC this
    # project can land on
    return load(name=_EXT_NAME, sources=_sources(), build_directory=build_dir,
                extra_cuda_cflags=["-O3", "-std=c++17", "-mavx2", "-mfma",
                                   "-mf16c", "-fopenmp"],
                extra_ldflags=["-L/opt/rocm/lib/llvm/lib", "-lomp",
                               "-Wl,-rpath,/opt/rocm/lib/llvm/lib"],
                verbose=verbose, with_cuda=True)


if __name__ == "__main__":
    load_extension(verbose=True)
    print("dllama_hip extension built OK")
