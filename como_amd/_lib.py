"""ctypes binding of libcomo_hip.so, derived from the C ABI declared in include/como_hip.h (_abi.py parses the header).

There is NO fallback: if the library or the header is missing or a call fails, the caller gets a RuntimeError.
torch is imported first so that the HIP runtime torch bundles (libamdhip64.so, soname .so.7) is the one
the library binds to -- one runtime, one set of streams.
"""
import ctypes
import os

import torch  # noqa: F401  (must precede CDLL: shares the HIP runtime)

from como_amd import _abi

_HERE = os.path.dirname(os.path.abspath(__file__))
# the same relative location csrc/ includes it from
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "como_hip.h")
# COMO_HIP_LIB: measurement scripts point this at the -DCOMO_AB_VARIANTS build (como_amd/lib_ab/libcomo_hip_ab.so); the product path
# is the in-tree library
LIB_PATH = os.environ.get("COMO_HIP_LIB") or os.path.join(_HERE, "lib", "libcomo_hip.so")
_lib = None


def _load_abi():
    try:
        with open(HEADER_PATH) as f:
            return _abi.parse(f.read())
    except (OSError, RuntimeError) as e:
        raise RuntimeError(f"como_amd: cannot derive the binding from {HEADER_PATH}: {e}") from e


# The binding is derived from the header the library is compiled against (mapping rule: _abi.py), once per process, at import.
# SIGNATURES: name -> (restype, argtypes) of every symbol include/como_hip.h declares; the Structures mirror its argument structs
_structs, SIGNATURES = _load_abi()
BAArgs, DRFuse, WinArgs = _structs["como_ba_args"], _structs["como_dr_fuse"], _structs["como_win_args"]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"como_amd: {LIB_PATH} is missing -- the HIP extension is not built. "
                "Run `python -m como_amd.build` (or __graft_entry__.build()). There is no CPU fallback.")
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f"como_amd: {what} failed with status {rc} "
                           f"({ {1: 'bad argument', 2: 'launch failure'}.get(rc, 'unknown') })")


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_dev_index = {}


def stream_ptr(device=None):
    """The current HIP stream of `device` as an integer handle.  Called before every launch (~25 times per eager GN iteration):
    torch's own raw accessor (0.3 us) instead of `torch.cuda.current_stream(device).cuda_stream` (5.6 us of Python per call)."""
    if _raw_stream is None:
        return torch.cuda.current_stream(device).cuda_stream
    idx = _dev_index.get(device)
    if idx is None:
        d = torch.device("cuda" if device is None else device)
        idx = d.index if d.index is not None else torch.cuda.current_device()
        if device is not None and torch.device(device).index is not None:
            _dev_index[device] = idx                        # (an explicit ordinal never changes; "cuda" follows the current device)
    return _raw_stream(idx)


def capture_graph(fn, device, thread_local=False):
    """Capture `fn()` into a hipGraph (torch.cuda.CUDAGraph).  Returns (graph, fn's result) or (None, error text): a capture
    that an operation inside invalidates leaves the capture stream in capture mode and torch's current stream pointing at it;
    both are undone here (como_abort_capture, stream restored), so the caller can go on launching eagerly.  After one such
    failure every later call returns (None, reason) at once."""
    global _capture_broken
    if _capture_broken:                        # torch's capture machinery does not survive an aborted capture (a second
        return None, _capture_broken           # attempt aborts the process): stay eager for the rest of the process
    prev = torch.cuda.current_stream(device)
    g = torch.cuda.CUDAGraph()
    ctx = torch.cuda.graph(g, capture_error_mode="thread_local" if thread_local else "global")
    try:
        with ctx:
            out = fn()
        return g, out
    except Exception:   # noqa: BLE001
        import traceback
        err = traceback.format_exc()[-1500:]
        cap = getattr(ctx, "capture_stream", None)
        for st in (cap, torch.cuda.current_stream(device)):
            if st is not None:
                lib().como_abort_capture(st.cuda_stream)
        torch.cuda.set_stream(prev)
        try:
            torch.cuda.synchronize(device)
        except Exception:   # noqa: BLE001
            pass
        lib().como_clear_last_error()
        _capture_broken = "graph capture disabled after an earlier capture failed: " + err[-300:]
        return None, err


_capture_broken = ""


def require_cuda(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("como_amd: tensors must live on the GPU (the HIP path has no CPU fallback)")


def suffix(dtype):
    if dtype == torch.float16:
        return "f16"
    if dtype == torch.float32:
        return "f32"
    if dtype == torch.float64:
        return "f64"
    raise RuntimeError(f"como_amd: unsupported dtype {dtype}")
