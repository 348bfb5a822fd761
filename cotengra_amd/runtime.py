"""ctypes binding of ``libctg_hip.so`` (C ABI: ``include/ctg_hip.h``).

The HIP library is the only execution engine: if it is missing this module
raises immediately -- there is no CPU fallback anywhere in the package.
"""

from __future__ import annotations

import collections
import ctypes as C
import operator
import os

import numpy as np

_LIB_PATH = os.environ.get("CTG_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libctg_hip.so")
ABI_VERSION = 10

# every symbol include/ctg_hip.h declares
SYMBOLS = (
    "ctg_abi_version",
    "ctg_last_error",
    "ctg_plan_create",
    "ctg_plan_destroy",
    "ctg_plan_nslices",
    "ctg_plan_workspace_bytes",
    "ctg_exec_create",
    "ctg_exec_destroy",
    "ctg_exec_set_stream",
    "ctg_exec_upload_inputs_host",
    "ctg_exec_upload_inputs_device",
    "ctg_exec_zero_result",
    "ctg_exec_set_strip_exponent",
    "ctg_exec_set_stem_arithmetic",
    "ctg_exec_get_exponent",
    "ctg_exec_run_slices",
    "ctg_exec_run_slice_list",
    "ctg_plan_share_units",
    "ctg_plan_share_slice_ids",
    "ctg_exec_run_share",
    "ctg_exec_slice_batch",
    "ctg_exec_device_bytes",
    "ctg_stem_triple_instantiated",
    "ctg_exec_launch_count",
    "ctg_exec_profile_slice",
    "ctg_exec_step_kernel",
    "ctg_exec_lds_form",
    "ctg_exec_step_paired_stores",
    "ctg_exec_step_stem_max",
    "ctg_plan_stem_pair16",
    "ctg_exec_sync",
    "ctg_exec_result_ptr",
    "ctg_exec_result_stats",
    "ctg_exec_sample_result",
    "ctg_exec_sample_info",
    "ctg_exec_range_audit",
    "ctg_exec_result_topk",
    "ctg_exec_result_marginal",
    "ctg_exec_result_rdm",
    "ctg_exec_result_rdm_wide",
    "ctg_rdm_wide_plan",
    "ctg_exec_result_pauli",
    "ctg_exec_result_pauli_apply",
    "ctg_exec_result_op_apply",
    "ctg_exec_result_pauli_spectrum",
    "ctg_pauli_spectrum_plan",
    "ctg_exec_result_cost",
    "ctg_cost_plan",
    "ctg_exec_download_result",
    "ctg_exec_download_arena",
    "ctg_exec_get_state",
    "ctg_exec_set_state",
    "ctg_exec_state_dtype",
    "ctg_exec_get_state_wide",
    "ctg_exec_set_state_wide",
    "ctg_comm_get_unique_id",
    "ctg_comm_init",
    "ctg_comm_info",
    "ctg_comm_destroy",
    "ctg_exec_reduce",
    "ctg_path_greedy",
    "ctg_slice_greedy",
    "ctg_subtree_reconfigure",
    "ctg_subtree_reconfigure_timed",
)


class CtgError(RuntimeError):
    """A call into libctg_hip.so failed."""


class CommError(CtgError):
    """RCCL is missing or a collective failed (CTG_E_COMM)."""


class PlanDesc(C.Structure):
    """Mirror of ``ctg_plan_desc``."""

    _fields_ = [
        ("dtype", C.c_int32),
        ("n_inputs", C.c_int64),
        ("input_sizes", C.POINTER(C.c_int64)),
        ("input_offsets", C.POINTER(C.c_int64)),
        ("inputs_elems", C.c_int64),
        ("arena_elems", C.c_int64),
        ("result_elems", C.c_int64),
        ("n_steps", C.c_int64),
        ("steps", C.POINTER(C.c_int64)),
        ("n_table_words", C.c_int64),
        ("tables", C.POINTER(C.c_int64)),
        ("n_sliced", C.c_int64),
        ("slice_sizes", C.POINTER(C.c_int64)),
        ("slice_fixed", C.POINTER(C.c_int64)),
        ("slice_strides", C.POINTER(C.c_int64)),
        ("slice_group", C.POINTER(C.c_int64)),
    ]


_lib = None


def lib_path():
    return _LIB_PATH


def load():
    """Load the shared library (once) and declare its prototypes."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(_LIB_PATH):
        raise ImportError(
            f"{_LIB_PATH} not found: build the HIP extension first "
            "(python -c 'import __graft_entry__ as g; g.build()'). "
            "cotengra_amd has no CPU fallback."
        )
    # PyTorch bundles its own libamdhip64.  The host layer uses torch for device
    # tensors, streams and RCCL, so torch's runtime must be the one this library
    # binds to: loading ours first would bring a second HIP runtime into the
    # process ("no ROCm-capable device" on the later one).
    try:
        import torch  # noqa: F401
    except ImportError:
        pass
    lib = C.CDLL(_LIB_PATH)
    i64p = C.POINTER(C.c_int64)
    vp = C.c_void_p
    lib.ctg_abi_version.restype = C.c_int
    lib.ctg_last_error.restype = C.c_char_p
    protos = {
        "ctg_plan_create": [C.POINTER(PlanDesc), C.POINTER(vp)],
        "ctg_plan_destroy": [vp],
        "ctg_plan_nslices": [vp, i64p],
        "ctg_plan_workspace_bytes": [vp, i64p],
        "ctg_exec_create": [vp, C.c_int, vp, vp, C.POINTER(vp)],
        "ctg_exec_destroy": [vp],
        "ctg_exec_set_stream": [vp, vp],
        "ctg_exec_upload_inputs_host": [vp, C.POINTER(vp)],
        "ctg_exec_upload_inputs_device": [vp, C.POINTER(vp)],
        "ctg_exec_zero_result": [vp],
        "ctg_exec_set_strip_exponent": [vp, C.c_int, C.c_int],
        "ctg_exec_set_stem_arithmetic": [vp, C.c_int],
        "ctg_exec_get_exponent": [vp, C.POINTER(C.c_double), C.POINTER(C.c_int)],
        "ctg_exec_run_slices": [vp, C.c_int64, C.c_int64, C.c_int64],
        "ctg_exec_run_slice_list": [vp, i64p, C.c_int64],
        "ctg_plan_share_units": [vp, C.c_int64, C.c_int64, i64p, i64p],
        "ctg_plan_share_slice_ids": [vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, i64p],
        "ctg_exec_run_share": [vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64],
        "ctg_exec_slice_batch": [vp, i64p],
        "ctg_exec_device_bytes": [vp, i64p],
        "ctg_stem_triple_instantiated": [C.c_int] * 9,
        "ctg_exec_launch_count": [vp, i64p, i64p],
        "ctg_exec_profile_slice": [vp, C.c_int64, C.POINTER(C.c_float)],
        "ctg_exec_step_kernel": [vp, C.c_int64, C.c_char_p, C.c_int64],
        "ctg_exec_lds_form": [vp, C.c_int64, C.c_int64, i64p, C.c_char_p, C.c_int64],
        "ctg_exec_step_paired_stores": [vp, C.c_int64, C.POINTER(C.c_int)],
        "ctg_exec_step_stem_max": [vp, C.c_int64, C.c_int64, C.POINTER(C.c_float)],
        "ctg_plan_stem_pair16": [vp, C.c_int64, C.POINTER(C.c_int)],
        "ctg_exec_sync": [vp],
        "ctg_exec_result_ptr": [vp, C.POINTER(vp)],
        "ctg_exec_result_stats": [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), i64p],
        "ctg_exec_sample_result": [vp, C.POINTER(C.c_double), C.c_int64, i64p, vp, C.POINTER(C.c_double)],
        "ctg_exec_sample_info": [vp, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), i64p,
                                 C.POINTER(C.c_float)],
        "ctg_exec_range_audit": [vp, C.c_int64, i64p, C.POINTER(C.c_double)],
        "ctg_exec_result_topk": [vp, C.c_int64, i64p, vp, C.POINTER(C.c_double)],
        "ctg_exec_result_marginal": [vp, C.c_int64, i64p, C.POINTER(C.c_int32), C.POINTER(C.c_double)],
        "ctg_exec_result_rdm": [vp, C.c_int64, i64p, C.POINTER(C.c_int32), vp],
        "ctg_exec_result_rdm_wide": [vp, C.c_int64, i64p, C.POINTER(C.c_int32), vp, C.POINTER(C.c_double)],
        "ctg_rdm_wide_plan": [C.c_int32, C.c_int64, i64p, C.POINTER(C.c_int32), i64p],
        "ctg_exec_result_pauli": [vp, C.c_int64, i64p, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(C.c_double)],
        "ctg_exec_result_pauli_apply": [vp, C.c_int64, i64p, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(C.c_double), vp, vp],
        "ctg_exec_result_op_apply": [vp, C.c_int64, i64p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                     C.POINTER(C.c_double), vp, vp],
        "ctg_exec_result_pauli_spectrum": [vp, C.c_int64, i64p, C.POINTER(C.c_uint8), C.c_int64, i64p,
                                           C.POINTER(C.c_double), vp],
        "ctg_pauli_spectrum_plan": [C.c_int32, C.c_int64, i64p, C.POINTER(C.c_uint8), i64p],
        "ctg_exec_result_cost": [vp, C.c_int64, i64p, C.c_int64, C.POINTER(C.c_uint8), C.POINTER(C.c_double), vp, C.c_int32,
                                 C.c_int64, C.POINTER(C.c_double), C.c_int64, C.POINTER(C.c_double), i64p, i64p, vp],
        "ctg_cost_plan": [C.c_int32, C.c_int64, i64p, C.c_int32, C.c_int64, C.c_int64, i64p],
        "ctg_exec_download_result": [vp, vp],
        "ctg_exec_download_arena": [vp, C.c_int64, C.c_int64, vp],
        "ctg_exec_get_state": [vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_int)],
        "ctg_exec_set_state": [vp, vp, C.c_double, C.c_int],
        "ctg_exec_state_dtype": [vp, C.POINTER(C.c_int)],
        "ctg_exec_get_state_wide": [vp, vp, C.POINTER(C.c_double), C.POINTER(C.c_int)],
        "ctg_exec_set_state_wide": [vp, vp, C.c_double, C.c_int],
        "ctg_comm_get_unique_id": [vp],
        "ctg_comm_init": [vp, C.c_int, C.c_int, C.c_int, C.POINTER(vp)],
        "ctg_comm_info": [vp, C.POINTER(C.c_int), C.POINTER(C.c_int), C.POINTER(C.c_int)],
        "ctg_comm_destroy": [vp],
        "ctg_exec_reduce": [vp, vp, C.c_int],
        "ctg_path_greedy": [C.c_int64, i64p, i64p, C.c_int64, i64p, C.c_int64, C.POINTER(C.c_double),
                            C.c_double, C.c_double, C.c_int64, C.c_uint64, i64p],
        "ctg_slice_greedy": [C.c_int64, i64p, i64p, C.c_int64, i64p, C.c_int64, C.POINTER(C.c_double),
                             i64p, C.c_double, C.c_int, C.c_int64, i64p, i64p],
        "ctg_subtree_reconfigure": [C.c_int64, i64p, i64p, C.c_int64, i64p, C.c_int64, C.POINTER(C.c_double),
                                    i64p, C.c_int64, C.c_int64, C.c_double, i64p],
        "ctg_subtree_reconfigure_timed": [C.c_int64, i64p, i64p, C.c_int64, i64p, C.c_int64,
                                          C.POINTER(C.c_double), i64p, C.c_int64, C.c_int64,
                                          C.POINTER(C.c_double), C.c_int64, C.c_double, i64p],
    }
    for name, argtypes in protos.items():
        fn = getattr(lib, name)
        fn.argtypes = argtypes
        fn.restype = C.c_int
    if lib.ctg_abi_version() != ABI_VERSION:
        raise ImportError(
            f"libctg_hip.so ABI {lib.ctg_abi_version()} != expected {ABI_VERSION}; rebuild."
        )
    _lib = lib
    return lib


def _check(rc):
    if rc != 0:
        msg = load().ctg_last_error().decode("utf-8", "replace")
        if rc in (-1, -6):   # (CTG_E_INVALID; CTG_E_NORM: nothing to draw from)
            raise ValueError(msg)
        if rc == -3:
            raise MemoryError(msg)
        if rc == -5:
            raise CommError(msg)
        raise CtgError(f"[{rc}] {msg}")


def _i64p(arr):
    return arr.ctypes.data_as(C.POINTER(C.c_int64))


def check_topk_k(k):
    """``k`` of a top-k request as an int: ``TypeError`` unless it is an integer (bool excluded), ``ValueError``
    below 1 -- host only, before any device work."""
    import operator

    if isinstance(k, (bool, np.bool_)):
        raise TypeError(f"k = {k!r} is not an integer.")
    try:
        k = operator.index(k)
    except TypeError:
        raise TypeError(f"k = {k!r} is not an integer.") from None
    if k < 1:
        raise ValueError(f"k = {k}: need at least 1.")
    return k


def rdm_dim(extents, keep):
    """``D``, the product of the kept extents of a reduced-density-matrix request: ``ValueError`` for an extent below
    1 and for ``D`` above ``Executor.RDM_MAX_DIM`` -- host only, before any device work."""
    d = 1
    for n, f in zip(extents, keep):
        if n < 1:
            raise ValueError(f"extent {n} is not positive.")
        if f == 1:
            d *= int(n)
    if d > Executor.RDM_MAX_DIM:
        raise ValueError(f"rdm: the kept extents' product is {d}; at most {Executor.RDM_MAX_DIM} (CTG_RDM_MAX_DIM).")
    return d


def rdm_variant(dtype, extents, keep):
    """The kernel ``ctg_exec_result_rdm`` chooses for a result of ``dtype`` and shape ``extents`` with the axes
    ``keep`` kept -- a function of those alone (csrc/ctg_rdm.hip): ``"rdm_chunk_kernel<T,NT>"`` on the power-of-two
    route (every extent a power of two, at least 4096 elements; ``NT = max(D, 16) / 16``), ``"rdm_general_kernel<T>"``
    otherwise; ``T`` one of ``float``, ``double``, ``c64``, ``c128``."""
    t = {"float32": "float", "float64": "double", "complex64": "c64", "complex128": "c128"}[np.dtype(dtype).name]
    ext = [int(n) for n in extents]
    d = rdm_dim(ext, list(keep))
    n = 1
    for v in ext:
        n *= v
    if n >= 4096 and all(v & (v - 1) == 0 for v in ext):
        return f"rdm_chunk_kernel<{t},{max(d, 16) // 16}>"
    return f"rdm_general_kernel<{t}>"


_DTYPE_TAG = {"float32": "float", "float64": "double", "complex64": "c64", "complex128": "c128"}
_DTYPE_CODE = {"float32": 0, "float64": 1, "complex64": 2, "complex128": 3}   # CTG_F32 .. CTG_C128


def rdm_wide_dim(extents, keep):
    """``D``, the product of the kept extents of a wide reduced-density-matrix request: ``ValueError`` for an extent
    below 1, for ``D`` up to ``Executor.RDM_MAX_DIM`` (those are ``rdm_result``'s: one route per ``D``) and for ``D``
    above ``Executor.RDM_WIDE_MAX_DIM`` -- host only, before any device work."""
    d = 1
    for n, f in zip(extents, keep):
        if n < 1:
            raise ValueError(f"extent {n} is not positive.")
        if f == 1:
            d *= int(n)
    if d <= Executor.RDM_MAX_DIM:
        raise ValueError(f"rdm_wide: the kept extents' product is {d}; up to {Executor.RDM_MAX_DIM} (CTG_RDM_MAX_DIM) "
                         "it is rdm_result (ctg_exec_result_rdm) that computes the matrix.")
    if d > Executor.RDM_WIDE_MAX_DIM:
        raise ValueError(f"rdm_wide: the kept extents' product is {d}; at most {Executor.RDM_WIDE_MAX_DIM} "
                         "(CTG_RDM_WIDE_MAX_DIM).")
    return d


RdmWidePlan = collections.namedtuple(
    "RdmWidePlan", "route dim edge panels blocks splits cols chunks grid scratch_bytes name_code")
RdmWidePlan.__doc__ = """The words of ``ctg_rdm_wide_plan`` (include/ctg_hip.h): ``route`` 0 power of two, 1 general;
``dim`` = D; ``edge`` rows of a row panel; ``panels``; ``blocks`` of the lower triangle (block ``bi (bi + 1) / 2 + bj`` is
panel ``bi`` times panel ``bj``); ``splits`` along r (split ``s`` takes the chunks ``s chunks / splits`` up to
``(s + 1) chunks / splits``); ``cols`` values of r per chunk; ``chunks``; ``grid`` = blocks * splits; ``scratch_bytes``;
``name_code`` = 4 * route + dtype code."""


def rdm_wide_scratch_bound(d):
    """``CTG_RDM_WIDE_SCRATCH_BYTES(D)`` of include/ctg_hip.h."""
    return 16 * d * d + max(8 * d * d + 512 * d, 64 << 20) + (64 << 10)


def _lowest_bits(mask, k):
    r = 0
    while k > 0 and mask:
        r |= mask & -mask
        mask &= mask - 1
        k -= 1
    return r


def rdm_wide_plan(dtype, extents, keep):
    """What ``ctg_exec_result_rdm_wide`` launches for a result of ``dtype`` and shape ``extents`` with the axes ``keep``
    kept, as an :class:`RdmWidePlan` -- a pure-Python mirror of ``ctg_rdm_wide_plan`` (csrc/ctg_rdm_wide.hip), word for
    word.  ``ValueError`` for what :func:`rdm_wide_dim` refuses and for a keep entry outside {0, 1}."""
    name = np.dtype(dtype).name
    code = _DTYPE_CODE[name]
    p = 2 if code >= 2 else 1
    ext = [int(v) for v in extents]
    kp = [int(f) for f in keep]
    if len(ext) != len(kp):
        raise ValueError(f"{len(ext)} extents and {len(kp)} keep entries.")
    for v, f in zip(ext, kp):
        if v < 1:
            raise ValueError(f"extent {v} is not positive.")
        if f not in (0, 1):
            raise ValueError("rdm_wide: a keep entry is neither 0 nor 1")
    d = rdm_wide_dim(ext, kp)
    n = 1
    for v in ext:
        n *= v
    if n > 1 << 40:
        raise ValueError("rdm_wide: the extents' product does not equal result_elems")
    t = n // d
    up256 = lambda b: (b + 255) & ~255   # noqa: E731
    pieces = (d * d + 4095) // 4096
    if n >= 4096 and all(v & (v - 1) == 0 for v in ext):
        route, edge = 0, 64
        mask, stride = 0, 1
        for v, f in zip(reversed(ext), reversed(kp)):
            if f:
                mask |= (v - 1) * stride
            stride *= v
        r = (n - 1) & ~mask
        rlo = _lowest_bits(r, 5)
        cols = 1 << bin(rlo).count("1")
        chunks = 1 << bin(r & ~rlo).count("1")
        panels = d // edge
        blocks = panels * (panels + 1) // 2
        splits = 1
        while blocks * splits < 512 and 2 * splits * 32 <= chunks:
            splits *= 2
        grid = blocks * splits
        part = grid * edge * edge * p * 8
    else:
        route, edge, panels = 1, 1, d
        blocks = d * (d + 1) // 2
        chunk = max(1024, (t + 1023) // 1024)
        cap = max(1, (64 << 20) // (blocks * p * 8))
        if (t + chunk - 1) // chunk > cap:
            chunk = (t + cap - 1) // cap
        cols = chunk
        chunks = (t + chunk - 1) // chunk
        splits = chunks
        grid = blocks * splits
        part = grid * p * 8
    scratch = up256(d * d * p * 8) + up256(part) + up256(pieces * 8) + up256(8)
    return RdmWidePlan(route, d, edge, panels, blocks, splits, cols, chunks, grid, scratch, 4 * route + code)


def rdm_wide_variant(dtype, extents, keep):
    """The kernel ``ctg_exec_result_rdm_wide`` chooses for a result of ``dtype`` and shape ``extents`` with the axes
    ``keep`` kept (csrc/ctg_rdm_wide.hip): ``"rdm_wide_kernel<T,64>"`` on the power-of-two route (every extent a power
    of two, at least 4096 elements; 64 the block edge), ``"rdm_wide_general_kernel<T>"`` otherwise; ``T`` one of
    ``float``, ``double``, ``c64``, ``c128``."""
    plan = rdm_wide_plan(dtype, extents, keep)
    t = _DTYPE_TAG[np.dtype(dtype).name]
    return f"rdm_wide_kernel<{t},{plan.edge}>" if plan.route == 0 else f"rdm_wide_general_kernel<{t}>"


def _pauli_ops(extents, ops):
    """``(extents as ints, n, ops as a C-contiguous uint8 (m, rank) array)`` of a Pauli request, validated as
    ``ctg_exec_result_pauli`` validates it -- host only: ``ValueError`` for an extent below 1, a row of the wrong
    length, a code above 3, a non-identity code on an axis whose extent is not 2 and more than
    ``Executor.PAULI_MAX_STRINGS`` strings."""
    ext = [int(v) for v in extents]
    n = 1
    for v in ext:
        if v < 1:
            raise ValueError(f"extent {v} is not positive.")
        n *= v
    raw = np.asarray(ops)
    if raw.size and raw.dtype.kind not in "iub":
        raise ValueError(f"pauli: codes of dtype {raw.dtype}; integers 0 .. 3 (I, X, Y, Z) are expected.")
    if raw.size and (raw.min() < 0 or raw.max() > 3):
        raise ValueError("pauli: a code is none of 0, 1, 2, 3 (I, X, Y, Z).")
    if raw.ndim == 1 and raw.size == len(ext) and len(ext) > 0:
        raw = raw.reshape(1, len(ext))
    if raw.ndim != 2 or raw.shape[1] != len(ext):
        raise ValueError(f"pauli: codes of shape {raw.shape}; (m, {len(ext)}) is expected, one column per axis.")
    arr = np.ascontiguousarray(raw, dtype=np.uint8)
    if arr.shape[0] > Executor.PAULI_MAX_STRINGS:
        raise ValueError(f"pauli: {arr.shape[0]} strings; at most {Executor.PAULI_MAX_STRINGS} (CTG_PAULI_MAX_STRINGS) "
                         "per call.")
    for a, v in enumerate(ext):
        if v != 2 and arr[:, a].any():
            raise ValueError(f"pauli: a letter other than I on axis {a} of extent {v}; only an axis of extent 2 "
                             "carries X, Y or Z.")
    return ext, n, arr


def _pauli_fast(ext, n):
    return n >= 4096 and all(v & (v - 1) == 0 for v in ext)


def pauli_masks(extents, ops):
    """``[(xm, zm, ny), ...]`` per string of ``ops`` (``(m, rank)`` codes 0 .. 3 = I, X, Y, Z over a tensor of shape
    ``extents``) as the power-of-two route of ``ctg_exec_result_pauli`` sees it: ``xm`` the flat-index bits of the X
    and Y axes, ``zm`` those of the Z and Y axes, ``ny`` the number of Y.  The flat bit of an axis is log2 of its
    row-major stride.  Host only; ``ValueError`` for what the call refuses and for an extent that is no power of
    two."""
    ext, n, arr = _pauli_ops(extents, ops)
    if any(v & (v - 1) for v in ext):
        raise ValueError(f"pauli_masks: the extents {tuple(ext)} are not all powers of two.")
    stride, s = [0] * len(ext), 1
    for a in range(len(ext) - 1, -1, -1):
        stride[a] = s
        s *= ext[a]
    out = []
    for row in arr.tolist():
        xm = zm = ny = 0
        for a, op in enumerate(row):
            if op in (1, 2):
                xm |= stride[a]
            if op in (2, 3):
                zm |= stride[a]
            ny += op == 2
        out.append((xm, zm, ny))
    return out


def pauli_variant(dtype, extents, ops):
    """The kernel ``ctg_exec_result_pauli`` runs for a result of ``dtype`` and shape ``extents`` and the strings
    ``ops`` -- a function of those alone (csrc/ctg_pauli.hip): ``"pauli_chunk_kernel<T>"`` on the power-of-two route
    (every extent a power of two, at least 4096 elements), ``"pauli_general_kernel<T>"`` otherwise; ``T`` one of
    ``float``, ``double``, ``c64``, ``c128``; ``"none"`` when every string is answered without a launch (no string,
    or a real ``dtype`` and an odd number of Y in every string)."""
    name = np.dtype(dtype).name
    t = _DTYPE_TAG[name]
    ext, n, arr = _pauli_ops(extents, ops)
    odd = (arr == 2).sum(axis=1) % 2 == 1
    if arr.shape[0] == 0 or (np.dtype(dtype).kind != "c" and bool(odd.all())):
        return "none"
    return f"pauli_chunk_kernel<{t}>" if _pauli_fast(ext, n) else f"pauli_general_kernel<{t}>"


PauliSpectrumPlan = collections.namedtuple(
    "PauliSpectrumPlan", "bits xm partner tile_bits passes pass_bits tiles scratch_bytes kernels")
PauliSpectrumPlan.__doc__ = """The words of ``ctg_pauli_spectrum_plan`` (include/ctg_hip.h): ``bits`` = L; ``xm`` the
flat-index mask of the flipped axes; ``partner`` 0 the element itself (``xm = 0``), 1 the thread's own 16-byte group, 2
another group of the chunk, 3 another chunk; ``tile_bits`` = min(L, 12); ``passes`` strided passes with ``pass_bits``
each; ``tiles`` workgroups of every launch; ``scratch_bytes`` of the vector when ``dev_out`` is not given; ``kernels``
the launches in order as the binding spells them, ``"spectrum_tile_kernel<T>"`` then ``"spectrum_pass_kernel"`` per
strided pass (``"spectrum_gather_kernel"`` follows when entries are selected)."""

PAULI_SPECTRUM_PLAN_WORDS = 12          # CTG_PAULI_SPECTRUM_PLAN_WORDS
PAULI_SPECTRUM_MAX_SELECT = 1 << 24     # CTG_PAULI_SPECTRUM_MAX_SELECT


def _spectrum_args(extents, flips):
    """``(extents int64, flips uint8)`` of a spectrum request, both with room for one entry at rank 0 -- host only:
    ``ValueError`` for another number of flips than extents and for a flip that is no integer in 0 .. 255 (what the
    codes mean is the library's to refuse)."""
    ext = np.zeros(max(len(extents), 1), dtype=np.int64)
    ext[:len(extents)] = [int(v) for v in extents]
    raw = np.asarray(flips).reshape(-1)
    if raw.size != len(extents):
        raise ValueError(f"pauli_spectrum: {len(extents)} extents and {raw.size} flips.")
    if raw.size and (raw.dtype.kind not in "iub" or raw.min() < 0 or raw.max() > 255):
        raise ValueError("pauli_spectrum: a flip is no integer code; 0 or 1 per axis is expected.")
    fl = np.zeros(max(len(extents), 1), dtype=np.uint8)
    fl[:raw.size] = raw
    return ext, fl


def pauli_spectrum_plan(dtype, extents, flips):
    """What ``ctg_exec_result_pauli_spectrum`` launches for a result of ``dtype`` and shape ``extents`` (every extent 1
    or 2) with the axes ``flips`` carrying X or Y, as a :class:`PauliSpectrumPlan` (``ctg_pauli_spectrum_plan``: host
    only, no device).  ``ValueError`` for what the call refuses of the shape and the flips."""
    name = np.dtype(dtype).name
    ext, fl = _spectrum_args(extents, flips)
    words = np.zeros(PAULI_SPECTRUM_PLAN_WORDS, dtype=np.int64)
    _check(load().ctg_pauli_spectrum_plan(_DTYPE_CODE[name], len(extents), _i64p(ext), fl.ctypes.data_as(C.POINTER(C.c_uint8)),
                                          _i64p(words)))
    w = words.tolist()
    kernels = (f"spectrum_tile_kernel<{_DTYPE_TAG[name]}>",) + ("spectrum_pass_kernel",) * w[4]
    return PauliSpectrumPlan(w[0], w[1], w[2], w[3], w[4], tuple(w[5:5 + w[4]]), w[9], w[10], kernels)


CostPlan = collections.namedtuple(
    "CostPlan", "bits n tile_bits passes pass_bits tiles digit_passes digit_launches grid scratch_bytes chunks hist_words kernels")
CostPlan.__doc__ = """The words of ``ctg_cost_plan`` (include/ctg_hip.h): ``bits`` = L for terms, -1 for values; ``n``
elements; ``tile_bits`` = min(L, 12); ``passes`` strided passes with ``pass_bits`` each; ``tiles`` workgroups of a
transform launch; ``digit_passes`` per level (6; 1 without levels) and ``digit_launches`` = 1 + 5 nl in all; ``grid``
workgroups of a digit pass and of the final pass; ``scratch_bytes`` with the vector in the scratch and no term table;
``chunks`` of 4096 elements; ``hist_words`` = ne + 1 (0 without edges); ``kernels`` the launches in order as the binding
spells them."""

COST_MAX_TERMS = 1 << 20     # CTG_COST_MAX_TERMS
COST_MAX_LEVELS = 8          # CTG_COST_MAX_LEVELS
COST_MAX_EDGES = 4097        # CTG_COST_MAX_EDGES
COST_WORDS = 64              # CTG_COST_WORDS
COST_LEVEL_WORD0 = 24        # CTG_COST_LEVEL_WORD0
COST_LEVEL_WORDS = 5         # CTG_COST_LEVEL_WORDS
COST_PLAN_WORDS = 16         # CTG_COST_PLAN_WORDS
COST_TERMS, COST_VALUES = 0, 1


def cost_plan(dtype, extents, source="terms", nl=0, ne=0):
    """What ``ctg_exec_result_cost`` launches for a result of ``dtype`` and shape ``extents``, the cost from ``source``
    (``"terms"``: every extent 1 or 2; ``"values"``: any extents), ``nl`` levels and ``ne`` edges, as a
    :class:`CostPlan` (``ctg_cost_plan``: host only, no device).  ``ValueError`` for what the call refuses of these."""
    name = np.dtype(dtype).name
    if source not in ("terms", "values"):
        raise ValueError(f"cost_plan: source = {source!r} is neither 'terms' nor 'values'.")
    ext = np.zeros(max(len(extents), 1), dtype=np.int64)
    ext[:len(extents)] = [int(v) for v in extents]
    words = np.zeros(COST_PLAN_WORDS, dtype=np.int64)
    _check(load().ctg_cost_plan(_DTYPE_CODE[name], len(extents), _i64p(ext), COST_TERMS if source == "terms" else COST_VALUES,
                                int(nl), int(ne), _i64p(words)))
    w = words.tolist()
    tag = _DTYPE_TAG[name]
    first = ("cost_scatter_kernel", "cost_tile_kernel") + ("cost_pass_kernel",) * w[3] if source == "terms" else ("cost_check_kernel",)
    digit = (f"cost_digit_kernel<{tag}>", "cost_rowsum_kernel", "cost_select_kernel")
    last = (f"cost_final_kernel<{tag},{1 if ne else 0}>",) + (("cost_rowsum_kernel",) if ne else ()) + ("cost_finish_kernel",)
    kernels = first + digit[:2] + (digit[2:] if nl else ()) + digit * (5 * int(nl)) + last
    return CostPlan(w[0], w[1], w[2], w[3], tuple(w[4:4 + w[3]]), w[8], w[9], w[10], w[11], w[12], w[14], w[15], kernels)


def cost_masks(extents, ops):
    """The flat-index mask of the Z axes per row of ``ops`` (``(m, rank)`` codes 0 = I and 3 = Z over a tensor of shape
    ``extents``, every extent 1 or 2), as an int64 array -- host only: what ``ctg_exec_result_cost`` forms.
    ``ValueError`` for another code, Z on an axis of extent 1 and an extent above 2."""
    ext = [int(v) for v in extents]
    if any(v < 1 or v > 2 for v in ext):
        raise ValueError(f"cost: the extents {tuple(ext)}; with terms every extent must be 1 or 2.")
    raw = np.asarray(ops)
    if raw.size and raw.dtype.kind not in "iub":
        raise ValueError(f"cost: codes of dtype {raw.dtype}; integers 0 (I) and 3 (Z) are expected.")
    arr = np.ascontiguousarray(raw, dtype=np.int64).reshape(-1, len(ext)) if len(ext) else np.zeros((int(raw.shape[0]) if raw.ndim else 0, 0), np.int64)
    if arr.size and not np.all((arr == 0) | (arr == 3)):
        raise ValueError("cost: a code is neither 0 (I) nor 3 (Z); X and Y terms are not a classical cost.")
    stride = np.ones(len(ext), dtype=np.int64)
    for a in range(len(ext) - 2, -1, -1):
        stride[a] = stride[a + 1] * ext[a + 1]
    for a, v in enumerate(ext):
        if v != 2 and arr[:, a].any():
            raise ValueError(f"cost: Z on axis {a} of extent {v}; only an axis of extent 2 carries Z.")
    return ((arr == 3).astype(np.int64) * stride[None, :]).sum(axis=1)


def pauli_apply_coeffs(coeffs, m):
    """``coeffs`` of a Pauli-sum request as a float64 ``(m,)`` array (``None``: ones) -- host only: ``ValueError`` for
    another length, a complex or non-numeric value and a coefficient that is not finite."""
    if coeffs is None:
        return np.ones(m, dtype=np.float64)
    raw = np.asarray(coeffs)
    if raw.dtype.kind not in "iufb":
        raise ValueError(f"pauli_apply: coefficients of dtype {raw.dtype}; real numbers are expected.")
    c = np.ascontiguousarray(raw, dtype=np.float64).reshape(-1)
    if c.size != m:
        raise ValueError(f"pauli_apply: {c.size} coefficients for {m} strings.")
    if not np.all(np.isfinite(c)):
        raise ValueError("pauli_apply: a coefficient is not finite.")
    return c


def pauli_apply_variant(dtype, extents, ops):
    """The kernel ``ctg_exec_result_pauli_apply`` runs for a result of ``dtype`` and shape ``extents`` and the strings
    ``ops`` -- a function of those alone (csrc/ctg_pauli_apply.hip): ``"pauli_apply_kernel<T>"`` on the power-of-two
    route (every extent a power of two, at least 4096 elements), ``"pauli_apply_general_kernel<T>"`` otherwise; ``T``
    one of ``float``, ``double``, ``c64``, ``c128``; ``"none"`` for no string (zeros are written without a kernel).
    ``ValueError`` for what the call refuses, a string with an odd number of Y on a real ``dtype`` included."""
    t = _DTYPE_TAG[np.dtype(dtype).name]
    ext, n, arr = _pauli_ops(extents, ops)
    if np.dtype(dtype).kind != "c" and bool(((arr == 2).sum(axis=1) % 2 == 1).any()):
        raise ValueError("pauli_apply: a string with an odd number of Y on a real tensor: P x is not real.")
    if arr.shape[0] == 0:
        return "none"
    return f"pauli_apply_kernel<{t}>" if _pauli_fast(ext, n) else f"pauli_apply_general_kernel<{t}>"


OP_MAX_DIM = 64            # CTG_OP_MAX_DIM
OP_MAX_TERMS = 4096        # CTG_OP_MAX_TERMS
OP_MAX_ENTRIES = 1 << 20   # CTG_OP_MAX_ENTRIES


def op_apply_terms(dtype, extents, terms):
    """The terms of a dense-operator request, checked and packed as ``ctg_exec_result_op_apply`` takes them -- host
    only.  ``terms``: a sequence of ``(axes, matrix)``; ``axes`` distinct positions in ``extents`` in ascending order,
    ``matrix`` of shape ``(D, D)`` with ``D`` the product of those extents, rows and columns row-major over the axes.
    Returns ``(extents as ints, naxes int32 (m,), axes int32 (sum naxes,), mats float64 (sum D^2, 2))``.  ``ValueError``
    -- before any device work -- for everything the C call would refuse: an extent below 1, more than
    ``OP_MAX_TERMS`` terms, a term without axes, an axis out of range, repeated or not ascending, ``D`` above
    ``OP_MAX_DIM``, a matrix of another shape, more than ``OP_MAX_ENTRIES`` entries in all, an entry that is not
    finite and, for a real ``dtype``, a non-zero imaginary part."""
    ext = [int(v) for v in extents]
    for v in ext:
        if v < 1:
            raise ValueError(f"extent {v} is not positive.")
    real = np.dtype(dtype).kind != "c"
    terms = list(terms)
    if len(terms) > OP_MAX_TERMS:
        raise ValueError(f"op_apply: {len(terms)} terms; at most {OP_MAX_TERMS} (CTG_OP_MAX_TERMS) per call.")
    naxes, axes, mats, entries = [], [], [], 0
    for t, term in enumerate(terms):
        try:
            if not isinstance(term, (tuple, list)):
                raise TypeError
            ax, mat = term
            ax = [operator.index(a) for a in ax]
        except (TypeError, ValueError):
            raise ValueError(f"op_apply: term {t} is no (axes, matrix) pair.") from None
        if not ax:
            raise ValueError(f"op_apply: term {t} names no axis.")
        d = 1
        for q, a in enumerate(ax):
            if a < 0 or a >= len(ext):
                raise ValueError(f"op_apply: term {t}: axis {a} is outside the rank {len(ext)}.")
            if q and a <= ax[q - 1]:
                raise ValueError(f"op_apply: term {t}: its axes {ax} are not ascending and distinct.")
            d *= ext[a]
        if d > OP_MAX_DIM:
            raise ValueError(f"op_apply: term {t}: the product of its extents is {d}; at most {OP_MAX_DIM} (CTG_OP_MAX_DIM).")
        raw = np.asarray(mat)
        if raw.dtype.kind not in "iufbc":
            raise ValueError(f"op_apply: term {t}: a matrix of dtype {raw.dtype}; numbers are expected.")
        if raw.shape != (d, d):
            raise ValueError(f"op_apply: term {t}: a matrix of shape {raw.shape}; ({d}, {d}) is expected.")
        o = np.ascontiguousarray(raw, dtype=np.complex128)
        if not np.all(np.isfinite(o.view(np.float64))):
            raise ValueError(f"op_apply: term {t}: a matrix entry is not finite.")
        if real and np.any(o.imag != 0.0):
            raise ValueError(f"op_apply: term {t}: a matrix entry has an imaginary part: O x of a real tensor is not real.")
        entries += d * d
        if entries > OP_MAX_ENTRIES:
            raise ValueError(f"op_apply: more than {OP_MAX_ENTRIES} (CTG_OP_MAX_ENTRIES) matrix entries in all.")
        naxes.append(len(ax))
        axes.extend(ax)
        mats.append(o.view(np.float64).reshape(-1, 2))
    packed = np.concatenate(mats) if mats else np.zeros((0, 2), dtype=np.float64)
    return (ext, np.asarray(naxes, dtype=np.int32), np.asarray(axes, dtype=np.int32),
            np.ascontiguousarray(packed, dtype=np.float64))


def op_apply_variant(dtype, extents, terms):
    """The kernel ``ctg_exec_result_op_apply`` runs for a result of ``dtype`` and shape ``extents`` and the ``terms``
    (:func:`op_apply_terms`) -- a function of those alone (csrc/ctg_op_apply.hip): ``"op_apply_kernel<T>"`` on the
    power-of-two route (every extent a power of two, at least 4096 elements), ``"op_apply_general_kernel<T>"``
    otherwise; ``T`` one of ``float``, ``double``, ``c64``, ``c128``; ``"none"`` for no term (zeros are written
    without a kernel).  ``ValueError`` for what the call refuses."""
    t = _DTYPE_TAG[np.dtype(dtype).name]
    ext, naxes, axes, mats = op_apply_terms(dtype, extents, terms)
    if naxes.size == 0:
        return "none"
    n = 1
    for v in ext:
        n *= v
    return f"op_apply_kernel<{t}>" if _pauli_fast(ext, n) else f"op_apply_general_kernel<{t}>"


class DevicePlan:
    """A validated plan inside the native library (host memory only)."""

    def __init__(self, plan):
        self.plan = plan
        lib = load()
        s = plan.serialise()
        self._keep = s  # the C side deep-copies, but keep until created
        d = PlanDesc()
        d.dtype = s["dtype"]
        d.n_inputs = len(s["input_sizes"])
        d.input_sizes = _i64p(s["input_sizes"])
        d.input_offsets = _i64p(s["input_offsets"])
        d.inputs_elems = plan.inputs_elems
        d.arena_elems = s["arena_elems"]
        d.result_elems = s["result_elems"]
        d.n_steps = s["n_steps"]
        d.steps = _i64p(s["steps"])
        d.n_table_words = len(s["tables"])
        d.tables = _i64p(s["tables"])
        d.n_sliced = len(s["slice_sizes"])
        d.slice_sizes = _i64p(s["slice_sizes"])
        d.slice_fixed = _i64p(s["slice_fixed"])
        d.slice_strides = _i64p(s["slice_strides"])
        d.slice_group = _i64p(s["slice_group"])
        handle = C.c_void_p()
        _check(lib.ctg_plan_create(C.byref(d), C.byref(handle)))
        self.handle = handle
        self._keep = None

    @property
    def nslices(self):
        n = C.c_int64()
        _check(load().ctg_plan_nslices(self.handle, C.byref(n)))
        return n.value

    def stem_pair16(self):
        """Per plan step: is it a stem pair whose result's tables allow 16-byte stores of two adjacent columns
        (``ctg_plan_stem_pair16``)?  No device needed."""
        fn = load().ctg_plan_stem_pair16
        out = []
        for s in range(len(self.plan.steps)):
            v = C.c_int()
            _check(fn(self.handle, s, C.byref(v)))
            out.append(bool(v.value))
        return out

    def share_units(self, rank=0, world=1):
        """``(units, slices per unit)`` of ``rank``'s share (``ctg_plan_share_units``): whole slice
        groups ``rank, rank + world, ...``; single slices for a plan without group indices."""
        u, g = C.c_int64(), C.c_int64()
        _check(load().ctg_plan_share_units(self.handle, int(rank), int(world), C.byref(u), C.byref(g)))
        return u.value, g.value

    def share_slice_ids(self, rank=0, world=1, unit_first=0, unit_count=-1):
        """Slice ids of the units ``[unit_first, unit_first + unit_count)`` of ``rank``'s share."""
        units, gsize = self.share_units(rank, world)
        n = units - unit_first if unit_count < 0 else unit_count
        out = np.empty(max(n, 0) * gsize, dtype=np.int64)
        _check(load().ctg_plan_share_slice_ids(self.handle, int(rank), int(world), int(unit_first), int(n), _i64p(out)))
        return out

    def workspace_bytes(self):
        out = (C.c_int64 * 4)()
        _check(load().ctg_plan_workspace_bytes(self.handle, out))
        return dict(zip(("inputs", "arena", "result", "tables"), out))

    def close(self):
        if getattr(self, "handle", None):
            load().ctg_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Executor:
    """One GPU's resident state for a plan: inputs, arena, tables, result."""

    def __init__(self, dplan, device=0, stream=0, result_ptr=None):
        self.dplan = dplan
        self.plan = dplan.plan
        self.device = int(device)
        handle = C.c_void_p()
        _check(
            load().ctg_exec_create(
                dplan.handle,
                self.device,
                C.c_void_p(int(stream) if stream else None),
                C.c_void_p(int(result_ptr) if result_ptr else None),
                C.byref(handle),
            )
        )
        self.handle = handle

    def set_stream(self, stream):
        """Enqueue all later work on ``stream`` (a raw ``hipStream_t`` value)."""
        _check(load().ctg_exec_set_stream(self.handle, C.c_void_p(int(stream) if stream else None)))

    # -- inputs ---------------------------------------------------------- #

    def upload_host(self, arrays):
        """``arrays``: numpy arrays; converted to the plan dtype, C order."""
        dt = np.dtype(self.plan.dtype)
        keep = [np.ascontiguousarray(x, dtype=dt) for x in arrays]
        self._check_sizes([x.size for x in keep])
        ptrs = (C.c_void_p * len(keep))(*[x.ctypes.data for x in keep])
        _check(load().ctg_exec_upload_inputs_host(self.handle, ptrs))

    def upload_device(self, ptrs, sizes):
        """``ptrs``: raw device addresses of contiguous tensors already in the
        plan dtype."""
        self._check_sizes(sizes)
        arr = (C.c_void_p * len(ptrs))(*[int(p) for p in ptrs])
        _check(load().ctg_exec_upload_inputs_device(self.handle, arr))

    def _check_sizes(self, sizes):
        want = list(self.plan.input_sizes)
        if list(sizes) != want:
            raise ValueError(
                f"Input sizes {list(sizes)} do not match the plan's {want}."
            )

    # -- execution --------------------------------------------------------- #

    def zero_result(self):
        _check(load().ctg_exec_zero_result(self.handle))

    def set_strip_exponent(self, strip, check_zero=False):
        _check(load().ctg_exec_set_strip_exponent(self.handle, int(bool(strip)), int(bool(check_zero))))

    STEM_ARITHMETICS = {"fp32": 0, "bf16x3": 1, "fp16x2": 2}

    def set_stem_arithmetic(self, mode):
        """Arithmetic of the fused stem pairs (include/ctg_hip.h): ``"fp32"`` / ``False`` / 0 -- fp32 products on
        the fp32 matrix cores; ``"bf16x3"`` / 1 -- operands split exactly into three bf16 limbs, six products;
        ``"fp16x2"`` / 2 -- two fp16 limbs under per-tensor power-of-two scales, three products (the
        executor's default since round 6).  ``True`` keeps its old meaning, ``"bf16x3"``."""
        if mode is True:
            mode = 1
        elif mode is False:
            mode = 0
        elif isinstance(mode, str):
            mode = self.STEM_ARITHMETICS[mode]
        _check(load().ctg_exec_set_stem_arithmetic(self.handle, int(mode)))

    def get_exponent(self):
        e, z = C.c_double(), C.c_int()
        _check(load().ctg_exec_get_exponent(self.handle, C.byref(e), C.byref(z)))
        return e.value, bool(z.value)

    def run_slice_list(self, ids):
        """Contract the slices ``ids`` (any order, any subset) and add them to the result; with slice
        groups in the plan, group by group (``ctg_exec_run_slice_list``)."""
        arr = np.ascontiguousarray(ids, dtype=np.int64)
        _check(load().ctg_exec_run_slice_list(self.handle, arr.ctypes.data_as(C.POINTER(C.c_int64)), arr.size))

    def run_share(self, rank=0, world=1, unit_first=0, unit_count=-1):
        """Contract units ``[unit_first, unit_first + unit_count)`` of ``rank``'s share of the slices
        (``ctg_exec_run_share``: whole slice groups ``rank, rank + world, ...``; the round-robin of
        ``contract_mpi``, core.py:4070, for a plan without groups) and add them to the result."""
        _check(load().ctg_exec_run_share(self.handle, int(rank), int(world), int(unit_first), int(unit_count)))

    def run_slices(self, first=0, count=None, stride=1):
        if count is None:
            count = (self.plan.nslices - first + stride - 1) // stride
        _check(load().ctg_exec_run_slices(self.handle, first, count, stride))

    @property
    def batch(self):
        """Slices that share one launch sequence in ``run_slices`` (1 for wide trees)."""
        n = C.c_int64()
        _check(load().ctg_exec_slice_batch(self.handle, C.byref(n)))
        return n.value

    def device_bytes(self):
        """Device memory the executor holds (arena x slice batch, inputs, tables, result,
        scratch): ``ctg_exec_device_bytes``."""
        n = C.c_int64()
        _check(load().ctg_exec_device_bytes(self.handle, C.byref(n)))
        return n.value

    def launch_count(self):
        """``(steps, launches)`` of one slice: independent small steps share launches."""
        ns, nl = C.c_int64(), C.c_int64()
        _check(load().ctg_exec_launch_count(self.handle, C.byref(ns), C.byref(nl)))
        return ns.value, nl.value

    def profile_slice(self, slice_id=0):
        ms = (C.c_float * max(len(self.plan.steps), 1))()
        _check(load().ctg_exec_profile_slice(self.handle, slice_id, ms))
        return np.asarray(ms[: len(self.plan.steps)], dtype=np.float64)

    def step_kernels(self):
        """Kernel name per plan step (as rocprof reports it, shortened)."""
        buf = C.create_string_buffer(160)
        names = []
        for s in range(len(self.plan.steps)):
            _check(load().ctg_exec_step_kernel(self.handle, s, buf, 160))
            names.append(buf.value.decode())
        return names

    def lds_forms(self):
        """Per packed LDS-resident subtree (the ``c`` of ``lds_run_kernel[c]`` in :meth:`step_kernels`), in the order
        its workgroup walks them, one ``(name, step)`` per shadow record: the form the record takes inside the launch
        (``ctg_exec_lds_form``: ``load<gather|sum>``, ``pair<1|2|4>`` or ``pair_mfma<cols|rows>``; ``wave=W`` or
        ``all``, matrix-core records ``all rot=R``; ``shift`` or ``magic``) and the plan step it belongs to.  A subtree
        the packer left off is not in the list."""
        fn = load().ctg_exec_lds_form
        buf = C.create_string_buffer(96)
        main = C.c_int64()
        out = []
        while True:
            recs = []
            while True:
                _check(fn(self.handle, len(out), len(recs), C.byref(main), buf, 96))
                if main.value < 0:
                    break
                recs.append((buf.value.decode(), int(main.value)))
            if not recs:
                return out
            out.append(recs)

    def step_paired_stores(self):
        """Per plan step: did its last launch store two adjacent columns of a row as one 16-byte store
        (``ctg_exec_step_paired_stores``: the kernel ``stem2h_kernel_p16`` of a trace)?"""
        fn = load().ctg_exec_step_paired_stores
        out = []
        for s in range(len(self.plan.steps)):
            v = C.c_int()
            _check(fn(self.handle, s, C.byref(v)))
            out.append(bool(v.value))
        return out

    def step_stem_max(self, step, z=0):
        """The largest |component| the last launch of stem step ``step`` recorded of its result (``ctg_exec_step_stem_max``)."""
        v = C.c_float()
        _check(load().ctg_exec_step_stem_max(self.handle, int(step), int(z), C.byref(v)))
        return float(v.value)

    def sync(self):
        _check(load().ctg_exec_sync(self.handle))

    def result_ptr(self):
        p = C.c_void_p()
        _check(load().ctg_exec_result_ptr(self.handle, C.byref(p)))
        return p.value

    def download_result(self):
        out = np.empty(self.plan.result_shape, dtype=np.dtype(self.plan.dtype))
        _check(load().ctg_exec_download_result(self.handle, C.c_void_p(out.ctypes.data)))
        return out

    # -- statistics of / draws from the result tensor (csrc/ctg_sample.hip) -- #

    def result_stats(self):
        """``(sum p, sum p^2, max p, argmax)`` of ``p = |x|^2`` over the result tensor, summed in double on the
        device (``ctg_exec_result_stats``); the mantissa's values under ``strip_exponent``."""
        s, q, m, i = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        _check(load().ctg_exec_result_stats(self.handle, C.byref(s), C.byref(q), C.byref(m), C.byref(i)))
        return s.value, q.value, m.value, i.value

    def sample_result(self, uniforms):
        """One draw from ``p / sum p`` per uniform in ``[0, 1)`` by inverse CDF on the device
        (``ctg_exec_sample_result``): ``(flat indices, the elements there, their p)``.  ``ValueError`` for a
        uniform outside ``[0, 1)`` (nothing is launched) and for a result whose ``sum p`` is zero or not finite."""
        u = np.ascontiguousarray(uniforms, dtype=np.float64).reshape(-1)
        n = u.size
        idx = np.empty(n, dtype=np.int64)
        elems = np.empty(n, dtype=np.dtype(self.plan.dtype))
        p = np.empty(n, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        _check(load().ctg_exec_sample_result(self.handle, u.ctypes.data_as(dp), n, _i64p(idx),
                                             C.c_void_p(elems.ctypes.data), p.ctypes.data_as(dp)))
        return idx, elems, p

    def sample_info(self):
        """``(sum p, sum p^2, max p, argmax, (pass 1 ms, pass 2 ms))`` of the last ``result_stats`` /
        ``sample_result`` call -- the tensor as it was then -- without touching the device
        (``ctg_exec_sample_info``)."""
        s, q, m, i = C.c_double(), C.c_double(), C.c_double(), C.c_int64()
        ms = (C.c_float * 2)()
        _check(load().ctg_exec_sample_info(self.handle, C.byref(s), C.byref(q), C.byref(m), C.byref(i), ms))
        return s.value, q.value, m.value, i.value, (ms[0], ms[1])

    # -- top-k and marginals of the result tensor (csrc/ctg_reduce.hip) -- #

    TOPK_MAX = 1 << 20   # CTG_TOPK_MAX

    def topk_result(self, k):
        """The ``k`` most probable members of the result tensor (``ctg_exec_result_topk``): ``(flat indices, the
        elements there, their p)`` in the order ``p`` descending, the lower index first among equal ``p`` -- numpy's
        ``lexsort((index, -p))[:k]``, exactly.  ``ValueError`` for ``k < 1``, ``k`` above the number of elements or
        above ``TOPK_MAX`` (nothing is launched) and for a result whose ``sum p`` is not finite."""
        k = check_topk_k(k)
        idx = np.empty(k, dtype=np.int64)
        elems = np.empty(k, dtype=np.dtype(self.plan.dtype))
        p = np.empty(k, dtype=np.float64)
        _check(load().ctg_exec_result_topk(self.handle, k, _i64p(idx), C.c_void_p(elems.ctypes.data),
                                           p.ctypes.data_as(C.POINTER(C.c_double))))
        return idx, elems, p

    def marginal_result(self, extents, keep):
        """``out[j] = sum p`` over the elements of the result tensor whose kept coordinates are ``j``
        (``ctg_exec_result_marginal``): ``extents`` is the shape of the result, ``keep[a]`` 0 or 1 per axis; a flat
        float64 array, row-major over the kept axes in the tensor's own order.  ``ValueError`` for a wrong product of
        the extents, a keep entry outside {0, 1} and for a result whose ``sum p`` is not finite."""
        ext = np.ascontiguousarray(extents, dtype=np.int64).reshape(-1)
        kp = np.ascontiguousarray(keep, dtype=np.int32).reshape(-1)
        if ext.size != kp.size:
            raise ValueError(f"{ext.size} extents and {kp.size} keep entries.")
        m = 1
        for d, f in zip(ext.tolist(), kp.tolist()):
            if d < 1:
                raise ValueError(f"extent {d} is not positive.")
            if f == 1:
                m *= d
        out = np.empty(m, dtype=np.float64)
        _check(load().ctg_exec_result_marginal(self.handle, ext.size, _i64p(ext), kp.ctypes.data_as(C.POINTER(C.c_int32)),
                                               out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    # -- reduced density matrices of the result tensor (csrc/ctg_rdm.hip) -- #

    RDM_MAX_DIM = 64   # CTG_RDM_MAX_DIM

    def rdm_result(self, extents, keep):
        """``rho[a, b] = sum over r of x[a, r] conj(x[b, r])`` of the result tensor (``ctg_exec_result_rdm``): ``a``,
        ``b`` over the axes with ``keep[a] = 1``, ``r`` over the others; ``extents`` is the shape of the result.  A
        ``(D, D)`` complex128 array (float64 for a real plan), rows and columns row-major over the kept axes in the
        tensor's own order; exactly Hermitian.  ``ValueError`` for what ``marginal_result`` refuses, for ``D`` above
        ``RDM_MAX_DIM`` (nothing is launched) and for a result whose ``sum p`` is not finite."""
        ext = np.ascontiguousarray(extents, dtype=np.int64).reshape(-1)
        kp = np.ascontiguousarray(keep, dtype=np.int32).reshape(-1)
        if ext.size != kp.size:
            raise ValueError(f"{ext.size} extents and {kp.size} keep entries.")
        d = rdm_dim(ext.tolist(), kp.tolist())
        cplx = np.dtype(self.plan.dtype).kind == "c"
        out = np.empty((d, d), dtype=np.complex128 if cplx else np.float64)
        _check(load().ctg_exec_result_rdm(self.handle, ext.size, _i64p(ext), kp.ctypes.data_as(C.POINTER(C.c_int32)),
                                          C.c_void_p(out.ctypes.data)))
        return out

    def rdm_variant(self, extents, keep):
        """The name of the kernel ``rdm_result(extents, keep)`` runs on this executor (:func:`rdm_variant`)."""
        return rdm_variant(self.plan.dtype, extents, keep)

    # -- reduced density matrices above RDM_MAX_DIM rows (csrc/ctg_rdm_wide.hip) -- #

    RDM_WIDE_MAX_DIM = 4096   # CTG_RDM_WIDE_MAX_DIM

    def rdm_wide_result(self, extents, keep, matrix=True):
        """``(rho, purity)`` of the result tensor for ``RDM_MAX_DIM < D <= RDM_WIDE_MAX_DIM`` kept values
        (``ctg_exec_result_rdm_wide``): ``rho`` as :meth:`rdm_result` defines it, or ``None`` with ``matrix=False``
        (nothing of the matrix is downloaded); ``purity = sum |rho[a, b]|^2`` summed in a fixed order on the device, not
        normalised, the same bits either way.  ``ValueError`` for what ``marginal_result`` refuses, for ``D`` outside
        that range (nothing is launched) and for a result whose ``sum p`` is not finite."""
        ext = np.ascontiguousarray(extents, dtype=np.int64).reshape(-1)
        kp = np.ascontiguousarray(keep, dtype=np.int32).reshape(-1)
        if ext.size != kp.size:
            raise ValueError(f"{ext.size} extents and {kp.size} keep entries.")
        d = rdm_wide_dim(ext.tolist(), kp.tolist())
        cplx = np.dtype(self.plan.dtype).kind == "c"
        out = np.empty((d, d), dtype=np.complex128 if cplx else np.float64) if matrix else None
        purity = C.c_double()
        _check(load().ctg_exec_result_rdm_wide(self.handle, ext.size, _i64p(ext), kp.ctypes.data_as(C.POINTER(C.c_int32)),
                                               C.c_void_p(out.ctypes.data if matrix else None), C.byref(purity)))
        return out, purity.value

    def rdm_wide_variant(self, extents, keep):
        """The name of the kernel ``rdm_wide_result(extents, keep)`` runs on this executor (:func:`rdm_wide_variant`)."""
        return rdm_wide_variant(self.plan.dtype, extents, keep)

    # -- expectation values of Pauli strings over the result tensor (csrc/ctg_pauli.hip) -- #

    PAULI_MAX_STRINGS = 4096   # CTG_PAULI_MAX_STRINGS

    def pauli_result(self, extents, ops):
        """``value(P) = sum over j of conj(x[j]) (P x)[j]`` of the result tensor for every Pauli string of ``ops``
        (``ctg_exec_result_pauli``): ``extents`` is the shape of the result, ``ops`` an ``(m, rank)`` array of codes
        0, 1, 2, 3 = I, X, Y, Z, one column per axis; an axis that is not I must have extent 2.  A float64 ``(m,)``
        array, NOT normalised (the all-identity string gives ``sum p``); for a real plan a string with an odd number
        of Y is exactly 0.0.  The bits of a value do not depend on the other strings of the call.  ``ValueError`` for
        a wrong product of the extents, a code above 3, a letter other than I on an axis of another extent, more than
        ``PAULI_MAX_STRINGS`` strings (nothing is launched) and for a result whose ``sum p`` is not finite."""
        ext, n, arr = _pauli_ops(extents, ops)
        e = np.ascontiguousarray(ext, dtype=np.int64).reshape(-1)
        out = np.zeros(arr.shape[0], dtype=np.float64)
        _check(load().ctg_exec_result_pauli(self.handle, e.size, _i64p(e), arr.shape[0],
                                            arr.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            out.ctypes.data_as(C.POINTER(C.c_double))))
        return out

    def pauli_variant(self, extents, ops):
        """The name of the kernel ``pauli_result(extents, ops)`` runs on this executor (:func:`pauli_variant`)."""
        return pauli_variant(self.plan.dtype, extents, ops)

    # -- all Pauli strings of one X / Y pattern by a Walsh-Hadamard transform (csrc/ctg_pauli_spectrum.hip) -- #

    PAULI_SPECTRUM_MAX_SELECT = PAULI_SPECTRUM_MAX_SELECT

    def pauli_spectrum(self, extents, flips, select=None, dev_out=None):
        """``S[z] = <x| P(xm, z) |x>`` of the result tensor for ALL ``z`` in ``[0, n)`` at once
        (``ctg_exec_result_pauli_spectrum``): ``extents`` is the shape of the result, every extent 1 or 2; ``flips`` 0
        or 1 per axis marks the axes that carry X or Y, ``xm`` is the mask of their flat-index bits.  ``P(xm, z)`` has Y
        on the bits of ``xm & z``, X on ``xm & ~z``, Z on ``z & ~xm``; its value is what :meth:`pauli_result` gives
        that string, NOT normalised, in other bits.  Without ``select``: a float64 array of shape ``extents`` (Z / Y on
        the axes where the coordinate is 1), or ``None`` when ``dev_out`` -- a device address of ``n`` doubles that
        does not overlap the result tensor -- takes it instead.  With ``select``, up to ``PAULI_SPECTRUM_MAX_SELECT``
        flat indices: ``S[select]`` as a float64 array, and ``dev_out``, if given, still receives all of ``S``.  The
        bits of an entry depend on (dtype, extents, flips, the tensor's bytes) alone.  ``ValueError`` for what the
        call refuses (nothing is launched) and for a result whose ``sum p`` is not finite."""
        ext, fl = _spectrum_args(extents, flips)
        sel = None
        if select is not None:
            raw = np.asarray(select)
            if raw.size and raw.dtype.kind not in "iu":
                raise ValueError(f"pauli_spectrum: select of dtype {raw.dtype}; flat indices are integers.")
            sel = np.ascontiguousarray(raw, dtype=np.int64).reshape(-1)
            out = np.zeros(sel.size, dtype=np.float64)
        else:
            out = None if dev_out else np.zeros(tuple(int(v) for v in extents), dtype=np.float64)
        dp = C.POINTER(C.c_double)
        _check(load().ctg_exec_result_pauli_spectrum(
            self.handle, len(extents), _i64p(ext), fl.ctypes.data_as(C.POINTER(C.c_uint8)), 0 if sel is None else sel.size,
            None if sel is None else _i64p(sel), None if out is None else out.ctypes.data_as(dp),
            C.c_void_p(int(dev_out) if dev_out else None)))
        return out

    def pauli_spectrum_plan(self, extents, flips):
        """What ``pauli_spectrum(extents, flips)`` launches on this executor (:func:`pauli_spectrum_plan`)."""
        return pauli_spectrum_plan(self.plan.dtype, extents, flips)

    # -- the distribution of a classical cost under p (csrc/ctg_cost.hip) -- #

    COST_MAX_TERMS = COST_MAX_TERMS
    COST_MAX_LEVELS = COST_MAX_LEVELS
    COST_MAX_EDGES = COST_MAX_EDGES

    def cost_result(self, extents, ops=None, coeffs=None, dev_cost=None, tail=-1, levels=(), edges=None, dev_cost_out=None):
        """The statistics of a classical cost ``C(z)`` under ``p = |x|^2`` of the result tensor
        (``ctg_exec_result_cost``): ``extents`` is the shape of the result.  The cost is either ``ops`` (``(m, rank)``
        codes 0 = I, 3 = Z, every extent 1 or 2) with ``m`` real ``coeffs``, ``C(z) = sum_s coeffs[s] (-1)^popcount(z &
        m_s)``, or ``dev_cost``, the device address of ``n`` doubles.  ``tail`` -1 (lower) or +1 (upper); up to
        ``COST_MAX_LEVELS`` ``levels`` in (0, 1]; ``edges`` none or 2 .. ``COST_MAX_EDGES`` ascending finite numbers;
        ``dev_cost_out`` a device address of ``n`` doubles that receives ``C``.  Returns ``(words, hist)``: the int64
        array of ``COST_WORDS`` words laid out as include/ctg_hip.h documents (``words.view(np.float64)`` for the double
        words) and the int64 array of ``len(edges) + 1`` integer masses (``None`` without edges).  ``ValueError`` for
        what the call refuses (nothing is launched) and for a result whose ``sum p`` is not finite."""
        ext = np.zeros(max(len(extents), 1), dtype=np.int64)
        ext[:len(extents)] = [int(v) for v in extents]
        rank = len(extents)
        dp, u8p = C.POINTER(C.c_double), C.POINTER(C.c_uint8)
        m, ops_p, co_p = 0, None, None
        if ops is not None or coeffs is not None:
            if ops is None or coeffs is None:
                raise ValueError("cost: terms need both ops and coeffs.")
            raw = np.asarray(ops)
            if raw.size and (raw.dtype.kind not in "iub" or raw.min() < 0 or raw.max() > 255):
                raise ValueError("cost: a code is no integer; 0 (I) or 3 (Z) per axis is expected.")
            co = pauli_apply_coeffs(coeffs, len(raw) if raw.ndim else 0)
            m = co.size
            if raw.size != m * rank:
                raise ValueError(f"cost: codes of shape {raw.shape}; ({m}, {rank}) is expected, one column per axis.")
            arr = np.zeros(max(m * rank, 1), dtype=np.uint8)
            arr[:m * rank] = raw.reshape(-1)
            cobuf = np.zeros(max(m, 1), dtype=np.float64)
            cobuf[:m] = co
            ops_p, co_p = arr.ctypes.data_as(u8p), cobuf.ctypes.data_as(dp)
        lev = np.ascontiguousarray(levels, dtype=np.float64).reshape(-1)
        levbuf = np.zeros(max(lev.size, 1), dtype=np.float64)
        levbuf[:lev.size] = lev
        ed = None if edges is None else np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        ne = 0 if ed is None else ed.size
        if ed is not None and ne == 0:
            raise ValueError("cost: no edge is given; at least 2 are expected.")
        hist = None if ed is None else np.zeros(ne + 1, dtype=np.int64)
        words = np.zeros(COST_WORDS, dtype=np.int64)
        if tail not in (-1, 1):
            raise ValueError(f"cost: tail = {tail!r} is neither -1 (lower) nor +1 (upper).")
        _check(load().ctg_exec_result_cost(
            self.handle, rank, _i64p(ext), m, ops_p, co_p, C.c_void_p(int(dev_cost) if dev_cost else None), int(tail), lev.size,
            levbuf.ctypes.data_as(dp), ne, None if ed is None else ed.ctypes.data_as(dp), _i64p(words),
            None if hist is None else _i64p(hist), C.c_void_p(int(dev_cost_out) if dev_cost_out else None)))
        return words, hist

    def cost_plan(self, extents, source="terms", nl=0, ne=0):
        """What ``cost_result`` launches on this executor (:func:`cost_plan`)."""
        return cost_plan(self.plan.dtype, extents, source, nl, ne)

    # -- a Pauli sum applied to the result tensor (csrc/ctg_pauli_apply.hip) -- #

    def pauli_apply_result(self, extents, ops, coeffs, out_ptr=None):
        """``y = (sum over s of coeffs[s] P_s) x`` of the result tensor ``x`` for the Pauli strings ``ops``
        (``ctg_exec_result_pauli_apply``): ``extents`` and ``ops`` as for :meth:`pauli_result`, ``coeffs`` ``m`` real
        numbers (``None``: ones).  Without ``out_ptr``: a numpy array of the result's shape and dtype.  With
        ``out_ptr``, a device address of ``result_elems`` elements that does not overlap the result tensor: ``y`` is
        written there and ``None`` returned.  The result tensor is not written.  ``ValueError`` for what
        :meth:`pauli_result` refuses, for coefficients of another length or not finite, on a real plan for a string
        with an odd number of Y (nothing is launched), and for a result whose ``sum p`` is not finite."""
        ext, n, arr = _pauli_ops(extents, ops)
        c = pauli_apply_coeffs(coeffs, arr.shape[0])
        pauli_apply_variant(self.plan.dtype, ext, arr)   # (odd Y on a real plan)
        e = np.ascontiguousarray(ext, dtype=np.int64).reshape(-1)
        out = None if out_ptr else np.empty(tuple(ext), dtype=np.dtype(self.plan.dtype))
        _check(load().ctg_exec_result_pauli_apply(
            self.handle, e.size, _i64p(e), arr.shape[0], arr.ctypes.data_as(C.POINTER(C.c_uint8)),
            c.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(int(out_ptr) if out_ptr else None),
            C.c_void_p(None if out is None else out.ctypes.data)))
        return out

    def pauli_apply_variant(self, extents, ops):
        """The name of the kernel ``pauli_apply_result(extents, ops, ...)`` runs on this executor
        (:func:`pauli_apply_variant`)."""
        return pauli_apply_variant(self.plan.dtype, extents, ops)

    # -- dense local operators applied to the result tensor (csrc/ctg_op_apply.hip) -- #

    OP_MAX_DIM = OP_MAX_DIM            # CTG_OP_MAX_DIM
    OP_MAX_TERMS = OP_MAX_TERMS        # CTG_OP_MAX_TERMS
    OP_MAX_ENTRIES = OP_MAX_ENTRIES    # CTG_OP_MAX_ENTRIES

    def op_apply_result(self, extents, terms, out_ptr=None):
        """``y = (sum over t of O_t (x) 1) x`` of the result tensor ``x`` for the dense ``terms``
        (``ctg_exec_result_op_apply``): ``extents`` is the shape of the result, ``terms`` a sequence of ``(axes,
        matrix)`` as for :func:`op_apply_terms`, axes of any extent.  Without ``out_ptr``: a numpy array of the
        result's shape and dtype.  With ``out_ptr``, a device address of ``result_elems`` elements that does not
        overlap the result tensor: ``y`` is written there and ``None`` returned.  The result tensor is not written.
        ``ValueError`` for what :func:`op_apply_terms` refuses (nothing is launched), a wrong product of the extents
        and for a result whose ``sum p`` is not finite."""
        ext, naxes, axes, mats = op_apply_terms(self.plan.dtype, extents, terms)
        fn = load().ctg_exec_result_op_apply
        e = np.ascontiguousarray(ext, dtype=np.int64).reshape(-1)
        out = None if out_ptr else np.empty(tuple(ext), dtype=np.dtype(self.plan.dtype))
        i32p = C.POINTER(C.c_int32)
        _check(fn(self.handle, e.size, _i64p(e), naxes.size, naxes.ctypes.data_as(i32p), axes.ctypes.data_as(i32p),
                  mats.ctypes.data_as(C.POINTER(C.c_double)), C.c_void_p(int(out_ptr) if out_ptr else None),
                  C.c_void_p(None if out is None else out.ctypes.data)))
        return out

    def op_apply_variant(self, extents, terms):
        """The name of the kernel ``op_apply_result(extents, terms)`` runs on this executor
        (:func:`op_apply_variant`)."""
        return op_apply_variant(self.plan.dtype, extents, terms)

    # -- range audit (csrc/ctg_range.hip, cotengra_amd/rangeaudit.py) -- #

    RANGE_WORDS = 260

    def range_audit(self, slice_id=0):
        """Run slice ``slice_id`` step by step in the executor's current arithmetic, adding it to the result as
        ``run_slices(slice_id, 1, 1)`` would, and read every tensor on the way (``ctg_exec_range_audit``):
        ``(rows, sumsq)`` with ``rows[(n_inputs + n_steps), 260]`` int64 -- status, component count, zeros, 0 and
        the 256 counts by biased fp32 exponent -- and ``sumsq[n_inputs + n_steps]`` float64; rows of the input
        tensors first, then one per plan step.  ``rangeaudit.summarise`` reads a row.  ``ValueError`` for a
        double-precision plan, under ``strip_exponent`` and for a slice outside the tree."""
        t = len(self.plan.input_sizes) + len(self.plan.steps)
        rows = np.zeros((t, self.RANGE_WORDS), dtype=np.int64)
        sumsq = np.zeros(t, dtype=np.float64)
        _check(load().ctg_exec_range_audit(self.handle, int(slice_id), _i64p(rows), sumsq.ctypes.data_as(C.POINTER(C.c_double))))
        return rows, sumsq

    # -- checkpoint state (include/ctg_hip.h: ctg_exec_get_state / set_state) -- #

    def get_state(self):
        """``(partial_result, exponent, zero)`` after synchronising: everything
        a sliced run has accumulated so far."""
        out = np.empty(self.plan.result_shape, dtype=np.dtype(self.plan.dtype))
        e, z = C.c_double(), C.c_int()
        _check(load().ctg_exec_get_state(self.handle, C.c_void_p(out.ctypes.data), C.byref(e), C.byref(z)))
        return out, e.value, bool(z.value)

    def set_state(self, result, exponent=0.0, zero=False):
        """Restore what ``get_state`` / ``get_state_wide`` returned (instead of ``zero_result``): an array in
        the executor's state dtype -- the double-precision running sum of a single-precision sliced tree --
        continues the sum with the bits an uninterrupted run would carry; one in the plan's own dtype restarts
        it from the rounded values."""
        arr = np.asarray(result)
        wide = self.state_dtype()
        if arr.dtype == wide and wide != np.dtype(self.plan.dtype):
            arr = np.ascontiguousarray(arr)
            fn = load().ctg_exec_set_state_wide
        else:
            arr = np.ascontiguousarray(arr, dtype=np.dtype(self.plan.dtype))
            fn = load().ctg_exec_set_state
        if arr.size != int(np.prod(self.plan.result_shape, dtype=np.int64)):
            raise ValueError(f"state has {arr.size} elements, the plan's result {self.plan.result_shape}")
        _check(fn(self.handle, C.c_void_p(arr.ctypes.data), float(exponent), int(bool(zero))))

    def state_dtype(self):
        """Element type of the running sum (``ctg_exec_state_dtype``): float64 / complex128 for a
        float32 / complex64 sliced tree, else the plan's dtype."""
        d = C.c_int()
        _check(load().ctg_exec_state_dtype(self.handle, C.byref(d)))
        return np.dtype(("float32", "float64", "complex64", "complex128")[d.value])

    def get_state_wide(self):
        """``(running sum in state_dtype, exponent, zero)``: what a checkpoint stores."""
        out = np.empty(self.plan.result_shape, dtype=self.state_dtype())
        e, z = C.c_double(), C.c_int()
        _check(load().ctg_exec_get_state_wide(self.handle, C.c_void_p(out.ctypes.data), C.byref(e), C.byref(z)))
        return out, e.value, bool(z.value)

    # -- multi-GPU ---------------------------------------------------------- #

    def reduce(self, comm, root=None):
        """Sum the ranks' result tensors in place with RCCL on this executor's
        stream (``root=None``: all-reduce).  Reference ``contract_mpi``'s
        ``Allreduce`` / ``Reduce`` (core.py:4081, 4089)."""
        _check(load().ctg_exec_reduce(self.handle, comm.handle, -1 if root is None else int(root)))

    def download_arena(self, offset, n):
        out = np.empty(n, dtype=np.dtype(self.plan.dtype))
        _check(
            load().ctg_exec_download_arena(
                self.handle, offset, n, C.c_void_p(out.ctypes.data)
            )
        )
        return out

    def close(self):
        if getattr(self, "handle", None):
            load().ctg_exec_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Comm:
    """An RCCL communicator behind the C ABI (``ctg_comm_*``): one per process
    and GPU.  ``Comm.unique_id()`` on one rank, the 128 bytes handed to the
    others by any channel, then ``Comm(id, rank, world, device)`` collectively."""

    @staticmethod
    def unique_id():
        buf = C.create_string_buffer(128)
        _check(load().ctg_comm_get_unique_id(buf))
        return buf.raw

    def __init__(self, unique_id, rank, world, device=0):
        if len(unique_id) != 128:
            raise ValueError("unique id must be 128 bytes")
        handle = C.c_void_p()
        buf = C.create_string_buffer(bytes(unique_id), 128)
        _check(load().ctg_comm_init(buf, int(rank), int(world), int(device), C.byref(handle)))
        self.handle = handle
        self.rank, self.world, self.device = int(rank), int(world), int(device)

    @classmethod
    def from_torch_group(cls, group=None, device=None):
        """Create the communicator over the ranks of a ``torch.distributed``
        group, using the group only to hand the unique id around."""
        import torch
        import torch.distributed as dist

        rank, world = dist.get_rank(group), dist.get_world_size(group)
        box = [cls.unique_id() if rank == 0 else None]
        dist.broadcast_object_list(box, src=dist.get_global_rank(group, 0) if group is not None else 0, group=group)
        if device is None:
            device = torch.cuda.current_device()
        return cls(box[0], rank, world, device)

    def close(self):
        if getattr(self, "handle", None):
            load().ctg_comm_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
