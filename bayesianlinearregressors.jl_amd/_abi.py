"""ctypes binding of the C ABI in include/blr_mi355x.h (libblr_mi355x.so, hand-written HIP for gfx950).

There is NO CPU fallback: if the shared library has not been built, or no MI355X is visible when a
handle is requested, this module raises.  Build with ``python -c "import __graft_entry__ as g; g.build()"``
(or ``make -C bayesianlinearregressors.jl_amd/csrc``).
"""
from __future__ import annotations

import ctypes as C
import os
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("BLR_MI355X_LIB") or os.path.join(_HERE, "csrc", "libblr_mi355x.so")

LAYOUT_COLVECS, LAYOUT_ROWVECS = 0, 1
NOISE_ISOTROPIC, NOISE_DIAGONAL, NOISE_DENSE = 0, 1, 2
PRIOR_DENSE, PRIOR_UPPER_FACTOR, PRIOR_DIAGONAL = 0, 1, 2
MEM_HOST, MEM_DEVICE = 0, 1
# bits of Handle.get_stat("draw_route") (csrc/blr_host.hpp DrawRoute): the weights kernel, then the projection
DRAW_W_DIAG, DRAW_W_MFMA, DRAW_W_UVEC, DRAW_W_LARGE, DRAW_W_BATCHED_NS1, DRAW_W_BATCHED_NS4 = 1, 2, 4, 8, 16, 32
DRAW_P_FUSED, DRAW_P_SCALAR, DRAW_P_MFMA = 64, 128, 256
MULTI_COLS_PER_PASS = 64  # csrc/blr_multi.hpp kMultiColsPerPass: column slots of one pass of multi_cols_kernel (slot 0 = column 0)
MARG_COLS_PER_PASS = 16  # csrc/blr_marg_multi.hpp kMargColsPerPass: mean columns of one pass of marginals_cols_kernel
LOO_COLS_PER_PASS = 16  # csrc/blr_loo_multi.hpp kLooColsPerPass (= kMargColsPerPass): columns of one pass of loo_cols_kernel
STATE_COLS_PER_PASS = 16  # csrc/blr_state_cols.hpp kStateColsPerPass: columns of one pass of state_cols_kernel (column 0 is not among them)

_i64, _int, _vp = C.c_int64, C.c_int, C.c_void_p
_H = C.c_void_p


class BLRError(RuntimeError):
    """HIP/runtime failure or invalid argument reported by the library (negative return code)."""

    def __init__(self, code, msg):
        super().__init__(f"libblr_mi355x: code {code}: {msg}")
        self.code = code


class PosDefException(np.linalg.LinAlgError):
    """Mirrors LinearAlgebra.PosDefException(info): Cholesky broke at leading minor ``info``."""

    def __init__(self, info):
        super().__init__(f"matrix is not positive definite; Cholesky factorization failed (info = {info})")
        self.info = info


_SIGS = {
    "blr_abi_version": ([], _int),
    "blr_device_count": ([], _int),
    "blr_create": ([_int, C.POINTER(_H)], _int),
    "blr_destroy": ([_H], _int),
    "blr_last_error": ([_H], C.c_char_p),
    "blr_set_stream": ([_H, _vp], _int),
    "blr_reset_stream": ([_H], _int),
    "blr_set_async": ([_H, _int], _int),
    "blr_synchronize": ([_H], _int),
    "blr_set_option": ([_H, C.c_char_p, C.c_char_p], _int),
    "blr_release_workspace": ([_H], _int),
    "blr_last_route": ([_H], C.c_char_p),
    "blr_get_stat": ([_H, C.c_char_p, C.POINTER(_i64)], _int),
    "blr_reset_stats": ([_H], _int),
    "blr_device_alloc": ([_H, C.c_size_t, C.POINTER(_vp)], _int),
    "blr_device_free": ([_H, _vp], _int),
    "blr_memcpy_h2d": ([_H, _vp, _vp, C.c_size_t], _int),
    "blr_memcpy_d2h": ([_H, _vp, _vp, C.c_size_t], _int),
    "blr_timer_start": ([_H], _int),
    "blr_timer_stop": ([_H, C.POINTER(C.c_float)], _int),
    "blr_logpdf_sum": ([_H, _int, _i64, _vp, _vp], _int),
    "blr_comm_unique_id": ([_vp], _int),
    "blr_comm_init": ([_H, _int, _int, _vp], _int),
    "blr_comm_destroy": ([_H], _int),
    "blr_comm_size": ([_H], _int),
    "blr_comm_rank": ([_H], _int),
    "blr_logpdf_allgather_sum": ([_H, _i64, _vp, _vp, _vp], _int),
    "blr_allreduce_sum": ([_H, _int, _vp, _i64], _int),
    "blr_kfold_ragged_fold_offsets": ([_i64, _vp, _i64, _vp], _int),
    "blr_kfold_large_ragged_fold_sizes": ([_i64, _vp, _i64, _vp], _int),
    "blr_kfold_large_ragged_fold_offsets": ([_i64, _vp, _vp, _vp], _int),
}
for _suf in ("f64", "f32"):
    _SIGS[f"blr_posterior_batched_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _int, _vp, _i64, _int, _vp, _i64, _vp, _i64, _i64,
         _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp], _int)
    _SIGS[f"blr_posterior_ragged_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _vp, _vp, _i64, _vp, _int, _vp, _i64, _int, _vp, _i64, _vp, _i64, _i64,
         _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _vp], _int)
    _SIGS[f"blr_marginals_ragged_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _vp, _vp, _i64, _int, _vp, _i64, _int, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp], _int)
    _SIGS[f"blr_loo_ragged_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _vp, _vp, _i64, _vp, _int, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp], _int)
    _SIGS[f"blr_kfold_ragged_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _int, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp], _int)
    _SIGS[f"blr_kfold_large_ragged_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _vp, _vp, _vp, _i64, _vp, _int, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp], _int)
    _SIGS[f"blr_posterior_multi_batched_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _int, _vp, _i64, _int, _vp, _i64, _vp, _i64, _i64,
         _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _vp], _int)
    _SIGS[f"blr_posterior_nsharded_{_suf}"] = (
        [_H, _int, _i64, _i64, _i64, _vp, _i64, _vp, _int, _vp, _int, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _vp], _int)
    _SIGS[f"blr_update_factor_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _int, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _vp], _int)
    _SIGS[f"blr_downdate_factor_{_suf}"] = _SIGS[f"blr_update_factor_{_suf}"]  # the same signature
    _SIGS[f"blr_update_factor_ragged_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _vp, _vp, _i64, _vp, _int, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _vp], _int)
    _SIGS[f"blr_downdate_factor_ragged_{_suf}"] = _SIGS[f"blr_update_factor_ragged_{_suf}"]  # the same signature
    _SIGS[f"blr_update_multi_factor_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _int, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64,
         _vp, _i64, _vp], _int)
    _SIGS[f"blr_downdate_multi_factor_{_suf}"] = _SIGS[f"blr_update_multi_factor_{_suf}"]  # the same signature
    _SIGS[f"blr_loo_batched_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _int, _vp, _i64, _vp, _i64, _vp, _i64, _i64,
         _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp], _int)
    _SIGS[f"blr_kfold_batched_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _int, _vp, _i64, _vp, _i64, _vp, _i64, _i64,
         _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp], _int)
    _SIGS[f"blr_kfold_large_batched_{_suf}"] = _SIGS[f"blr_kfold_batched_{_suf}"]  # (the same argument list)
    _SIGS[f"blr_loo_multi_batched_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _int, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64,
         _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp], _int)
    _SIGS[f"blr_kfold_multi_batched_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _int, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _i64,
         _vp, _i64, _i64, _vp, _i64, _vp, _i64, _i64, _vp, _i64, _vp], _int)
    _SIGS[f"blr_logpdf_grid_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _int, _vp, _i64, _int, _vp, _i64, _vp, _i64, _i64,
         _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64], _int)
    _SIGS[f"blr_logpdf_grid_ragged_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _vp, _vp, _i64, _vp, _int, _vp, _i64, _int, _vp, _i64, _vp, _i64, _i64,
         _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _i64, _vp, _i64], _int)
    _SIGS[f"blr_posterior_{_suf}"] = (
        [_H, _int, _i64, _i64, _vp, _i64, _vp, _int, _vp, _int, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp], _int)
    _SIGS[f"blr_marginals_batched_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _vp, _i64, _i64, _int, _vp, _i64, _int, _vp, _i64, _vp, _i64, _i64,
         _vp, _i64, _vp, _i64, _vp], _int)
    _SIGS[f"blr_marginals_multi_batched_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _int, _vp, _i64, _int, _vp, _i64, _i64, _vp, _i64, _i64,
         _vp, _i64, _i64, _vp, _i64, _vp], _int)
    _SIGS[f"blr_rand_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _vp, _i64, _int, _vp, _int, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64], _int)
    _SIGS[f"blr_rand_batched_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _int, _vp, _i64, _int, _vp, _i64, _vp, _i64, _i64,
         _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp], _int)
    _SIGS[f"blr_rand_multi_batched_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _i64, _i64, _vp, _i64, _i64, _int, _vp, _i64, _int, _vp, _i64, _i64, _vp, _i64, _i64,
         _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _i64, _vp], _int)
    _SIGS[f"blr_apply_weights_{_suf}"] = ([_H, _int, _int, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64], _int)
    _SIGS[f"blr_sample_weights_{_suf}"] = (
        [_H, _int, _i64, _i64, _int, _vp, _vp, _i64, _vp, _i64, _vp, _i64], _int)
    _SIGS[f"blr_logpdf_grad_batched_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _vp, _i64, _i64, _vp, _i64, _int, _vp, _i64, _int, _vp, _i64, _vp, _i64, _i64,
         _vp, _vp, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _i64, _vp], _int)
    _SIGS[f"blr_logpdf_multi_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _int, _vp, _int, _vp, _vp, _i64, _vp, _vp, _i64, _vp], _int)
    _SIGS[f"blr_gram_stats_{_suf}"] = ([_H, _int, _i64, _i64, _vp, _i64, _vp, _int, _vp, _vp, _vp, _i64, _vp], _int)
    _SIGS[f"blr_posterior_from_stats_{_suf}"] = (
        [_H, _i64, _i64, _vp, _i64, _vp, _int, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp], _int)
    _SIGS[f"blr_posterior_dense_noise_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _vp, _i64, _vp, _vp, _i64, _int, _vp, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp], _int)
    _SIGS[f"blr_mean_and_cov_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _vp, _i64, _int, _vp, _i64, _int, _vp, _vp, _i64, _vp, _vp, _i64, _vp], _int)
    _SIGS[f"blr_mean_and_cov_batched_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _vp, _i64, _i64, _int, _vp, _i64, _i64, _int, _vp, _i64, _vp, _i64, _i64,
         _vp, _i64, _vp, _i64, _i64, _vp], _int)
    _SIGS[f"blr_rand_dense_noise_{_suf}"] = (
        [_H, _int, _int, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _int, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64], _int)
    _fp = C.c_double if _suf == "f64" else C.c_float
    _SIGS[f"blr_rff_features_{_suf}"] = (
        [_H, _int, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _fp, _vp, _i64], _int)
    _SIGS[f"blr_posterior_rff_{_suf}"] = (
        [_H, _int, _i64, _i64, _i64, _vp, _i64, _vp, _i64, _vp, _fp, _vp, _int, _vp, _int, _vp, _vp, _i64,
         _vp, _vp, _i64, _vp, _i64, _vp, _vp], _int)

EXPORTED_SYMBOLS = tuple(_SIGS)

_lib = None
_lib_lock = threading.Lock()


def load_library():
    """dlopen the HIP library (works without a GPU: only handle creation needs one)."""
    global _lib
    with _lib_lock:
        if _lib is None:
            if not os.path.exists(LIB_PATH):
                raise ImportError(
                    f"{LIB_PATH} is missing: the HIP extension has not been built. "
                    "Run `python -c 'import __graft_entry__ as g; g.build()'`. There is no CPU fallback."
                )
            if os.environ.get("BLR_MI355X_NO_TORCH_PRELOAD") != "1":
                # PyTorch wheels bundle their own libamdhip64/libhsa-runtime64.  Two HIP runtimes in one
                # process do not share the device ("No HIP GPUs are available" from whichever initialises
                # second), so when torch is installed let it load its runtime FIRST; our library then binds
                # to the already-loaded libamdhip64.so.  Without torch the system ROCm runtime is used.
                try:
                    import torch  # noqa: F401
                except Exception:
                    pass
            lib = C.CDLL(LIB_PATH)
            for name, (argtypes, restype) in _SIGS.items():
                fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
                fn.argtypes = argtypes
                fn.restype = restype
            _lib = lib
    return _lib


def _ptr(a):
    """void* of a numpy array, an int device pointer, or None."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data_as(_vp)
    return _vp(int(a))


def suffix(dtype):
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return "f64"
    if dtype == np.float32:
        return "f32"
    raise TypeError(f"unsupported element type {dtype}; the library is built for Float64 and Float32")


class Handle:
    """One library handle = one device + one stream + scratch.  Not thread-safe (one per thread)."""

    def __init__(self, device=0):
        self.lib = load_library()
        h = _H()
        rc = self.lib.blr_create(int(device), C.byref(h))
        if rc != 0:
            raise BLRError(rc, "blr_create failed: no usable MI355X/HIP device (the product path has no CPU fallback)")
        self._h = h
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self.lib.blr_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- error translation ---------------------------------------------------------------------
    def check(self, rc):
        if rc < 0:
            msg = self.lib.blr_last_error(self._h)
            raise BLRError(rc, msg.decode() if msg else "")
        return rc

    def set_stream(self, stream_ptr):
        """Run on the caller's hipStream_t (0 / None = the HIP null stream, torch's default stream)."""
        self.check(self.lib.blr_set_stream(self._h, _vp(int(stream_ptr)) if stream_ptr else None))
        self._caller_stream = (int(stream_ptr) if stream_ptr else 0,)

    def reset_stream(self):
        self.check(self.lib.blr_reset_stream(self._h))
        self._caller_stream = None

    def current_stream_setting(self):
        """None = the handle's own stream, else a 1-tuple holding the caller stream pointer (0 = the null stream)."""
        return getattr(self, "_caller_stream", None)

    def set_async(self, flag):
        self.check(self.lib.blr_set_async(self._h, int(bool(flag))))

    def synchronize(self):
        self.check(self.lib.blr_synchronize(self._h))

    def release_workspace(self):
        """Free the handle's grow-only device scratch (include/blr_mi355x.h blr_release_workspace)."""
        self.check(self.lib.blr_release_workspace(self._h))

    def set_option(self, key, value=None):
        """Run-time switch of this handle (include/blr_mi355x.h blr_set_option); value None = the built-in default.
        MAX_CHUNK = 1..65535 (tests) caps the regressors per chunk / slice of every batched entry point; RAGGED_ITEM = 1..2^30 (tests) forces
        the observations per work item of marginals_ragged / loo_ragged (rounded up to 64)."""
        self.check(self.lib.blr_set_option(self._h, str(key).encode(), None if value is None else str(value).encode()))

    def last_route(self):
        """Kernel family the most recent posterior / logpdf dispatch launched (include/blr_mi355x.h blr_last_route)."""
        return self.lib.blr_last_route(self._h).decode()

    def get_stat(self, key):
        """Counter of this handle: "i8_regressors", "i8_handed_back", "planes_redone", "loo_degenerate", "kfold_degenerate" (folds
        blr_kfold_batched_* / blr_kfold_multi_batched_* / blr_kfold_large_batched_* gave NaN), "workspace_bytes", "last_chunks" (chunks / slices of regressors of the most recent call: option MAX_CHUNK caps their size), "ragged_sweep" / "ragged_refit" / "ragged_idle" (regressors on each
        list of the most recent update_factor_ragged / downdate_factor_ragged call), and the variance route of the most recent
        marginals_batched call: "marg_block_rt" (tile height 32 / 16 of marg_blocksub_kernel, 0 = the call ran elsewhere), "marg_block_walk"
        (tiles its busiest workgroup walked), "marg_block_renumbered" (1 = a launch renumbered its workgroups per XCD), and the kernels of
        the most recent sample_weights / apply_weights / rand / rand_batched call: "draw_route", a bitmask of the DRAW_* constants of
        this module -- one weights bit (DRAW_W_UVEC rides on DRAW_W_MFMA: the 16-byte loader of the factor at D = 128) and at most one
        projection bit (none: no projection ran) (blr_get_stat)."""
        v = _i64()
        self.check(self.lib.blr_get_stat(self._h, str(key).encode(), C.byref(v)))
        return int(v.value)

    def reset_stats(self):
        self.check(self.lib.blr_reset_stats(self._h))

    def timer_start(self):
        self.check(self.lib.blr_timer_start(self._h))

    def timer_stop(self):
        ms = C.c_float()
        self.check(self.lib.blr_timer_stop(self._h, C.byref(ms)))
        return float(ms.value)

    # -- device memory (blr_device_alloc / blr_device_free / blr_memcpy_*): for hosts without a GPU array library ----------
    def device_alloc(self, nbytes):
        """-> integer device pointer (0 bytes -> 0)."""
        if nbytes <= 0:
            return 0
        p = _vp()
        self.check(self.lib.blr_device_alloc(self._h, C.c_size_t(int(nbytes)), C.byref(p)))
        return int(p.value or 0)

    def device_free(self, dptr):
        if dptr and getattr(self, "_h", None):
            self.check(self.lib.blr_device_free(self._h, _vp(int(dptr))))

    def memcpy_h2d(self, dptr, host_array):
        a = np.ascontiguousarray(host_array) if not (host_array.flags.c_contiguous or host_array.flags.f_contiguous) else host_array
        if a.nbytes:
            self.check(self.lib.blr_memcpy_h2d(self._h, _vp(int(dptr)), a.ctypes.data_as(_vp), C.c_size_t(a.nbytes)))

    def memcpy_d2h(self, host_array, dptr):
        if not (host_array.flags.c_contiguous or host_array.flags.f_contiguous):
            raise ValueError("memcpy_d2h needs a contiguous destination")
        if host_array.nbytes:
            self.check(self.lib.blr_memcpy_d2h(self._h, host_array.ctypes.data_as(_vp), _vp(int(dptr)), C.c_size_t(host_array.nbytes)))

    # -- raw entry points (see include/blr_mi355x.h for argument meaning) ---------------------------
    def posterior_batched(self, dtype, memspace, layout, B, D, N, X, ldx, strideX, y, stridey, noise_kind, s, strides,
                          prior_kind, mw, stridemw, Lw, ldl, strideLw, mw_post, stride_mwpost, T_post, ldt, strideT,
                          Lw_post, ldlp, strideLp, logpdf, info):
        fn = getattr(self.lib, f"blr_posterior_batched_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, N, _ptr(X), ldx, strideX, _ptr(y), stridey, noise_kind,
                             _ptr(s), strides, prior_kind, _ptr(mw), stridemw, _ptr(Lw), ldl, strideLw,
                             _ptr(mw_post), stride_mwpost, _ptr(T_post), ldt, strideT, _ptr(Lw_post), ldlp, strideLp,
                             _ptr(logpdf), _ptr(info)))

    def posterior_ragged(self, dtype, memspace, layout, B, D, offsets, X, ldx, y, noise_kind, s, strides, prior_kind, mw, stridemw,
                         Lw, ldl, strideLw, mw_post, stride_mwpost, T_post, ldt, strideT, Lw_post, ldlp, strideLp, logpdf, info):
        """B regressors with unequal observation counts, packed side by side, in one call; include/blr_mi355x.h
        blr_posterior_ragged_*.  offsets: B + 1 non-decreasing entries, always on the host (any integer sequence)."""
        fn = getattr(self.lib, f"blr_posterior_ragged_{suffix(dtype)}")
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.shape != (B + 1,):
            raise ValueError(f"offsets must have B + 1 = {B + 1} entries, got shape {offsets.shape}")
        return self.check(fn(self._h, memspace, layout, B, D, _ptr(offsets), _ptr(X), ldx, _ptr(y), noise_kind, _ptr(s), strides,
                             prior_kind, _ptr(mw), stridemw, _ptr(Lw), ldl, strideLw, _ptr(mw_post), stride_mwpost, _ptr(T_post),
                             ldt, strideT, _ptr(Lw_post), ldlp, strideLp, _ptr(logpdf), _ptr(info)))

    def marginals_ragged(self, dtype, memspace, layout, B, D, offsets, X, ldx, noise_kind, s, strides, prior_kind, mw, stridemw,
                         Lw, ldl, strideLw, mean, var, info):
        """Marginals of B regressors with unequal observation counts, inputs and outputs packed side by side; include/blr_mi355x.h
        blr_marginals_ragged_*.  offsets: B + 1 non-decreasing entries, always on the host (any integer sequence)."""
        fn = getattr(self.lib, f"blr_marginals_ragged_{suffix(dtype)}")
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.shape != (B + 1,):
            raise ValueError(f"offsets must have B + 1 = {B + 1} entries, got shape {offsets.shape}")
        return self.check(fn(self._h, memspace, layout, B, D, _ptr(offsets), _ptr(X), ldx, noise_kind, _ptr(s), strides, prior_kind,
                             _ptr(mw), stridemw, _ptr(Lw), ldl, strideLw, _ptr(mean), _ptr(var), _ptr(info)))

    def loo_ragged(self, dtype, memspace, layout, B, D, offsets, X, ldx, y, noise_kind, s, strides, mw, stridemw, T, ldt, strideT,
                   loo_mean, loo_var, loo_logpdf, loo_total, info):
        """Exact leave-one-out predictives of B states with unequal observation counts, packed as `posterior_ragged` packs them;
        include/blr_mi355x.h blr_loo_ragged_*."""
        fn = getattr(self.lib, f"blr_loo_ragged_{suffix(dtype)}")
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.shape != (B + 1,):
            raise ValueError(f"offsets must have B + 1 = {B + 1} entries, got shape {offsets.shape}")
        return self.check(fn(self._h, memspace, layout, B, D, _ptr(offsets), _ptr(X), ldx, _ptr(y), noise_kind, _ptr(s), strides,
                             _ptr(mw), stridemw, _ptr(T), ldt, strideT, _ptr(loo_mean), _ptr(loo_var), _ptr(loo_logpdf),
                             _ptr(loo_total), _ptr(info)))

    def kfold_ragged(self, dtype, memspace, layout, B, D, offsets, F, X, ldx, y, noise_kind, s, strides, mw, stridemw, T, ldt, strideT,
                     kf_mean, kf_var, kf_logpdf, kf_total, info):
        """Exact leave-fold-out predictives (folds of F <= 64 observations of each regressor's own slice) of B states with unequal
        observation counts, packed as `posterior_ragged` packs them; kf_logpdf is packed by folds (`kfold_ragged_fold_offsets`);
        include/blr_mi355x.h blr_kfold_ragged_*."""
        fn = getattr(self.lib, f"blr_kfold_ragged_{suffix(dtype)}")
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.shape != (B + 1,):
            raise ValueError(f"offsets must have B + 1 = {B + 1} entries, got shape {offsets.shape}")
        return self.check(fn(self._h, memspace, layout, B, D, _ptr(offsets), F, _ptr(X), ldx, _ptr(y), noise_kind, _ptr(s), strides,
                             _ptr(mw), stridemw, _ptr(T), ldt, strideT, _ptr(kf_mean), _ptr(kf_var), _ptr(kf_logpdf),
                             _ptr(kf_total), _ptr(info)))

    def kfold_large_ragged(self, dtype, memspace, layout, B, D, offsets, fold_sizes, X, ldx, y, noise_kind, s, strides, mw, stridemw, T, ldt,
                           strideT, kf_mean, kf_var, kf_logpdf, kf_total, info):
        """Exact leave-fold-out predictives for LARGE folds of B states with unequal observation counts, packed as `posterior_ragged`
        packs them: regressor b has folds of ``fold_sizes[b]`` observations of its own slice (an int: the same size for all);
        kf_logpdf is packed by folds (blr_kfold_large_ragged_fold_offsets); include/blr_mi355x.h blr_kfold_large_ragged_*."""
        fn = getattr(self.lib, f"blr_kfold_large_ragged_{suffix(dtype)}")
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.shape != (B + 1,):
            raise ValueError(f"offsets must have B + 1 = {B + 1} entries, got shape {offsets.shape}")
        fold_sizes = np.ascontiguousarray(np.broadcast_to(np.asarray(fold_sizes, dtype=np.int64), (B,)))
        return self.check(fn(self._h, memspace, layout, B, D, _ptr(offsets), _ptr(fold_sizes), _ptr(X), ldx, _ptr(y), noise_kind, _ptr(s),
                             strides, _ptr(mw), stridemw, _ptr(T), ldt, strideT, _ptr(kf_mean), _ptr(kf_var), _ptr(kf_logpdf),
                             _ptr(kf_total), _ptr(info)))

    def posterior_multi_batched(self, dtype, memspace, layout, B, D, N, S, X, ldx, strideX, Y, ldY, strideY, noise_kind, s, strides,
                                prior_kind, mw, stridemw, Lw, ldl, strideLw, mw_post, ldmp, stride_mwpost, T_post, ldt, strideT,
                                Lw_post, ldlp, strideLp, logpdf, stride_lp, info):
        """B regressors with S target columns each (Y: N x S per regressor) in one call: one factor per regressor, a mean and an
        evidence per column; include/blr_mi355x.h blr_posterior_multi_batched_* (one status per regressor in info)."""
        fn = getattr(self.lib, f"blr_posterior_multi_batched_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, N, S, _ptr(X), ldx, strideX, _ptr(Y), ldY, strideY, noise_kind, _ptr(s),
                             strides, prior_kind, _ptr(mw), stridemw, _ptr(Lw), ldl, strideLw, _ptr(mw_post), ldmp, stride_mwpost,
                             _ptr(T_post), ldt, strideT, _ptr(Lw_post), ldlp, strideLp, _ptr(logpdf), stride_lp, _ptr(info)))

    def posterior_nsharded(self, dtype, layout, D, N_local, N_total, X, ldx, y, noise_kind, s, prior_kind, mw, Lw, ldl, stats, lds,
                           scal, mw_post, T_post, ldt, Lw_post, ldlp, logpdf, info):
        """One regressor with its observations split over the ranks of comm_init (device pointers); blr_posterior_nsharded_*."""
        fn = getattr(self.lib, f"blr_posterior_nsharded_{suffix(dtype)}")
        return self.check(fn(self._h, layout, D, N_local, N_total, _ptr(X), ldx, _ptr(y), noise_kind, _ptr(s), prior_kind, _ptr(mw),
                             _ptr(Lw), ldl, _ptr(stats), lds, _ptr(scal), _ptr(mw_post), _ptr(T_post), ldt, _ptr(Lw_post), ldlp,
                             _ptr(logpdf), _ptr(info)))

    def update_factor(self, dtype, memspace, layout, B, D, k, X, ldx, strideX, y, stridey, noise_kind, s, strides, mw, stridemw,
                      T, ldt, strideT, logpdf, info):
        """In-place rank-k update of the resident state (mw, T); include/blr_mi355x.h blr_update_factor_*."""
        fn = getattr(self.lib, f"blr_update_factor_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, k, _ptr(X), ldx, strideX, _ptr(y), stridey, noise_kind, _ptr(s),
                             strides, _ptr(mw), stridemw, _ptr(T), ldt, strideT, _ptr(logpdf), _ptr(info)))

    def downdate_factor(self, dtype, memspace, layout, B, D, k, X, ldx, strideX, y, stridey, noise_kind, s, strides, mw, stridemw,
                        T, ldt, strideT, logpdf, info):
        """In-place rank-k downdate (forget observations) of the resident state (mw, T); include/blr_mi355x.h
        blr_downdate_factor_*."""
        fn = getattr(self.lib, f"blr_downdate_factor_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, k, _ptr(X), ldx, strideX, _ptr(y), stridey, noise_kind, _ptr(s),
                             strides, _ptr(mw), stridemw, _ptr(T), ldt, strideT, _ptr(logpdf), _ptr(info)))

    def _revise_ragged(self, name, dtype, memspace, layout, B, D, offsets, X, ldx, y, noise_kind, s, strides, mw, stridemw, T, ldt,
                       strideT, logpdf, info):
        fn = getattr(self.lib, f"blr_{name}_factor_ragged_{suffix(dtype)}")
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.shape != (B + 1,):
            raise ValueError(f"offsets must have B + 1 = {B + 1} entries, got shape {offsets.shape}")
        return self.check(fn(self._h, memspace, layout, B, D, _ptr(offsets), _ptr(X), ldx, _ptr(y), noise_kind, _ptr(s), strides,
                             _ptr(mw), stridemw, _ptr(T), ldt, strideT, _ptr(logpdf), _ptr(info)))

    def update_factor_ragged(self, dtype, memspace, layout, B, D, offsets, X, ldx, y, noise_kind, s, strides, mw, stridemw, T, ldt,
                             strideT, logpdf, info):
        """In-place update of B resident states (mw, T) that received unequal numbers of observations (none included), packed as
        `posterior_ragged` packs them; include/blr_mi355x.h blr_update_factor_ragged_*."""
        return self._revise_ragged("update", dtype, memspace, layout, B, D, offsets, X, ldx, y, noise_kind, s, strides, mw, stridemw,
                                   T, ldt, strideT, logpdf, info)

    def downdate_factor_ragged(self, dtype, memspace, layout, B, D, offsets, X, ldx, y, noise_kind, s, strides, mw, stridemw, T, ldt,
                               strideT, logpdf, info):
        """In-place downdate (forget observations) of B resident states (mw, T), unequal numbers of observations per state, packed as
        `posterior_ragged` packs them; include/blr_mi355x.h blr_downdate_factor_ragged_*."""
        return self._revise_ragged("downdate", dtype, memspace, layout, B, D, offsets, X, ldx, y, noise_kind, s, strides, mw, stridemw,
                                   T, ldt, strideT, logpdf, info)

    def update_multi_factor(self, dtype, memspace, layout, B, D, k, S, X, ldx, strideX, Y, ldY, strideY, noise_kind, s, strides, M, ldm,
                            strideM, T, ldt, strideT, logpdf, stride_lp, info):
        """In-place rank-k update of the resident multi-output state (M: D x S per regressor, one factor T); include/blr_mi355x.h
        blr_update_multi_factor_*."""
        fn = getattr(self.lib, f"blr_update_multi_factor_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, k, S, _ptr(X), ldx, strideX, _ptr(Y), ldY, strideY, noise_kind, _ptr(s),
                             strides, _ptr(M), ldm, strideM, _ptr(T), ldt, strideT, _ptr(logpdf), stride_lp, _ptr(info)))

    def downdate_multi_factor(self, dtype, memspace, layout, B, D, k, S, X, ldx, strideX, Y, ldY, strideY, noise_kind, s, strides, M,
                              ldm, strideM, T, ldt, strideT, logpdf, stride_lp, info):
        """In-place rank-k downdate (forget observations) of the resident multi-output state (M, T); include/blr_mi355x.h
        blr_downdate_multi_factor_*."""
        fn = getattr(self.lib, f"blr_downdate_multi_factor_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, k, S, _ptr(X), ldx, strideX, _ptr(Y), ldY, strideY, noise_kind, _ptr(s),
                             strides, _ptr(M), ldm, strideM, _ptr(T), ldt, strideT, _ptr(logpdf), stride_lp, _ptr(info)))

    def loo(self, dtype, memspace, layout, B, D, N, X, ldx, strideX, y, stridey, noise_kind, s, strides, mw, stridemw, T, ldt,
            strideT, loo_mean, stride_lm, loo_var, stride_lv, loo_logpdf, stride_ll, loo_total, info):
        """Exact leave-one-out predictives of the observations the states (mw, T) contain; include/blr_mi355x.h
        blr_loo_batched_*."""
        fn = getattr(self.lib, f"blr_loo_batched_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, N, _ptr(X), ldx, strideX, _ptr(y), stridey, noise_kind, _ptr(s),
                             strides, _ptr(mw), stridemw, _ptr(T), ldt, strideT, _ptr(loo_mean), stride_lm, _ptr(loo_var),
                             stride_lv, _ptr(loo_logpdf), stride_ll, _ptr(loo_total), _ptr(info)))

    def kfold(self, dtype, memspace, layout, B, D, N, F, X, ldx, strideX, y, stridey, noise_kind, s, strides, mw, stridemw, T, ldt,
              strideT, kf_mean, stride_km, kf_var, stride_kv, kf_logpdf, stride_kl, kf_total, info):
        """Exact leave-fold-out (K-fold) predictives of the observations the states (mw, T) contain, contiguous folds of F <= 64:
        mean and variance per observation, ONE joint log density per fold, one total per regressor; include/blr_mi355x.h
        blr_kfold_batched_*."""
        fn = getattr(self.lib, f"blr_kfold_batched_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, N, F, _ptr(X), ldx, strideX, _ptr(y), stridey, noise_kind, _ptr(s),
                             strides, _ptr(mw), stridemw, _ptr(T), ldt, strideT, _ptr(kf_mean), stride_km, _ptr(kf_var),
                             stride_kv, _ptr(kf_logpdf), stride_kl, _ptr(kf_total), _ptr(info)))

    def kfold_large(self, dtype, memspace, layout, B, D, N, F, X, ldx, strideX, y, stridey, noise_kind, s, strides, mw, stridemw, T,
                    ldt, strideT, kf_mean, stride_km, kf_var, stride_kv, kf_logpdf, stride_kl, kf_total, info):
        """The same predictives for LARGE folds, removed in weight space: any F >= 1 with ceil(N / F) <= 1024, D <= 128; arguments
        and outputs as `kfold`; include/blr_mi355x.h blr_kfold_large_batched_*."""
        fn = getattr(self.lib, f"blr_kfold_large_batched_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, N, F, _ptr(X), ldx, strideX, _ptr(y), stridey, noise_kind, _ptr(s),
                             strides, _ptr(mw), stridemw, _ptr(T), ldt, strideT, _ptr(kf_mean), stride_km, _ptr(kf_var),
                             stride_kv, _ptr(kf_logpdf), stride_kl, _ptr(kf_total), _ptr(info)))

    def loo_multi_batched(self, dtype, memspace, layout, B, D, N, S, X, ldx, strideX, Y, ldY, strideY, noise_kind, s, strides, M, ldm,
                          strideM, T, ldt, strideT, loo_mean, ld_lm, stride_lm, loo_var, stride_lv, loo_logpdf, ld_ll, stride_ll,
                          loo_total, stride_lt, info):
        """Exact leave-one-out predictives of the observations the multi-output states (M: D x S, T) contain: S means and log
        densities and ONE variance per input, S totals per regressor; include/blr_mi355x.h blr_loo_multi_batched_*."""
        fn = getattr(self.lib, f"blr_loo_multi_batched_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, N, S, _ptr(X), ldx, strideX, _ptr(Y), ldY, strideY, noise_kind, _ptr(s),
                             strides, _ptr(M), ldm, strideM, _ptr(T), ldt, strideT, _ptr(loo_mean), ld_lm, stride_lm, _ptr(loo_var),
                             stride_lv, _ptr(loo_logpdf), ld_ll, stride_ll, _ptr(loo_total), stride_lt, _ptr(info)))

    def kfold_multi_batched(self, dtype, memspace, layout, B, D, N, S, F, X, ldx, strideX, Y, ldY, strideY, noise_kind, s, strides, M,
                            ldm, strideM, T, ldt, strideT, kf_mean, ld_km, stride_km, kf_var, stride_kv, kf_logpdf, ld_kl, stride_kl,
                            kf_total, stride_kt, info):
        """Exact leave-fold-out (K-fold) predictives of the observations the multi-output states (M: D x S, T) contain, contiguous
        folds of F <= 64, D <= 128: S means per observation and ONE variance, S joint log densities per fold, S totals per regressor;
        include/blr_mi355x.h blr_kfold_multi_batched_*."""
        fn = getattr(self.lib, f"blr_kfold_multi_batched_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, N, S, F, _ptr(X), ldx, strideX, _ptr(Y), ldY, strideY, noise_kind, _ptr(s),
                             strides, _ptr(M), ldm, strideM, _ptr(T), ldt, strideT, _ptr(kf_mean), ld_km, stride_km, _ptr(kf_var),
                             stride_kv, _ptr(kf_logpdf), ld_kl, stride_kl, _ptr(kf_total), stride_kt, _ptr(info)))

    def logpdf_grid(self, dtype, memspace, layout, B, D, N, X, ldx, strideX, y, stridey, noise_kind, s, strides, prior_kind, mw,
                    stridemw, Lw, ldl, strideLw, G, alpha, stride_alpha, tau, stride_tau, logpdf, stride_lp, best, mw_best,
                    stride_mwbest, T_best, ldt, strideT, info, stride_info):
        """Evidence of every regressor under G settings (Lw = alpha Lw, s = tau s) from one pass over X, the best setting and
        its posterior; include/blr_mi355x.h blr_logpdf_grid_*."""
        fn = getattr(self.lib, f"blr_logpdf_grid_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, N, _ptr(X), ldx, strideX, _ptr(y), stridey, noise_kind, _ptr(s),
                             strides, prior_kind, _ptr(mw), stridemw, _ptr(Lw), ldl, strideLw, G, _ptr(alpha), stride_alpha,
                             _ptr(tau), stride_tau, _ptr(logpdf), stride_lp, _ptr(best), _ptr(mw_best), stride_mwbest,
                             _ptr(T_best), ldt, strideT, _ptr(info), stride_info))

    def logpdf_grid_ragged(self, dtype, memspace, layout, B, D, offsets, X, ldx, y, noise_kind, s, strides, prior_kind, mw, stridemw,
                           Lw, ldl, strideLw, G, alpha, stride_alpha, tau, stride_tau, logpdf, stride_lp, best, mw_best,
                           stride_mwbest, T_best, ldt, strideT, info, stride_info):
        """The evidence grid of B regressors with unequal observation counts, packed side by side, in one call; include/blr_mi355x.h
        blr_logpdf_grid_ragged_*.  offsets: B + 1 non-decreasing entries, always on the host (any integer sequence)."""
        fn = getattr(self.lib, f"blr_logpdf_grid_ragged_{suffix(dtype)}")
        offsets = np.ascontiguousarray(offsets, dtype=np.int64)
        if offsets.shape != (B + 1,):
            raise ValueError(f"offsets must have B + 1 = {B + 1} entries, got shape {offsets.shape}")
        return self.check(fn(self._h, memspace, layout, B, D, _ptr(offsets), _ptr(X), ldx, _ptr(y), noise_kind, _ptr(s), strides,
                             prior_kind, _ptr(mw), stridemw, _ptr(Lw), ldl, strideLw, G, _ptr(alpha), stride_alpha, _ptr(tau),
                             stride_tau, _ptr(logpdf), stride_lp, _ptr(best), _ptr(mw_best), stride_mwbest, _ptr(T_best), ldt,
                             strideT, _ptr(info), stride_info))

    def posterior(self, dtype, layout, D, N, X, ldx, y, noise_kind, s, prior_kind, mw, Lw, ldl, mw_post, T_post, ldt,
                  Lw_post, ldlp, logpdf):
        fn = getattr(self.lib, f"blr_posterior_{suffix(dtype)}")
        rc = self.check(fn(self._h, layout, D, N, _ptr(X), ldx, _ptr(y), noise_kind, _ptr(s), prior_kind, _ptr(mw),
                           _ptr(Lw), ldl, _ptr(mw_post), _ptr(T_post), ldt, _ptr(Lw_post), ldlp, _ptr(logpdf)))
        if rc > 0:
            raise PosDefException(rc)
        return rc

    def logpdf_grad_batched(self, dtype, memspace, layout, B, D, N, X, ldx, strideX, y, stridey, noise_kind, s, strides,
                            prior_kind, mw, stridemw, Lw, ldl, strideLw, logpdf, dX, lddx, stridedX, dy, stridedy, ds,
                            strideds, dmw, stridedmw, mw_post, stride_mwpost, Ainv, ldai, strideAi, info):
        fn = getattr(self.lib, f"blr_logpdf_grad_batched_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, N, _ptr(X), ldx, strideX, _ptr(y), stridey, noise_kind,
                             _ptr(s), strides, prior_kind, _ptr(mw), stridemw, _ptr(Lw), ldl, strideLw, _ptr(logpdf),
                             _ptr(dX), lddx, stridedX, _ptr(dy), stridedy, _ptr(ds), strideds, _ptr(dmw), stridedmw,
                             _ptr(mw_post), stride_mwpost, _ptr(Ainv), ldai, strideAi, _ptr(info)))

    def logpdf_multi(self, dtype, memspace, layout, D, N, S, X, ldx, Y, ldY, noise_kind, s, prior_kind, mw, Lw, ldl, logpdf,
                     mw_post, ldmp, info):
        fn = getattr(self.lib, f"blr_logpdf_multi_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, D, N, S, _ptr(X), ldx, _ptr(Y), ldY, noise_kind, _ptr(s), prior_kind,
                             _ptr(mw), _ptr(Lw), ldl, _ptr(logpdf), _ptr(mw_post), ldmp, _ptr(info)))

    def gram_stats(self, dtype, layout, D, N, X, ldx, y, noise_kind, s, mw, stats, lds, scal):
        fn = getattr(self.lib, f"blr_gram_stats_{suffix(dtype)}")
        return self.check(fn(self._h, layout, D, N, _ptr(X), ldx, _ptr(y), noise_kind, _ptr(s), _ptr(mw), _ptr(stats), lds, _ptr(scal)))

    def posterior_from_stats(self, dtype, D, N_total, stats, lds, scal, prior_kind, mw, Lw, ldl, mw_post, T_post, ldt, Lw_post,
                             ldlp, logpdf, info):
        fn = getattr(self.lib, f"blr_posterior_from_stats_{suffix(dtype)}")
        return self.check(fn(self._h, D, N_total, _ptr(stats), lds, _ptr(scal), prior_kind, _ptr(mw), _ptr(Lw), ldl,
                             _ptr(mw_post), _ptr(T_post), ldt, _ptr(Lw_post), ldlp, _ptr(logpdf), _ptr(info)))

    def marginals_batched(self, dtype, memspace, layout, B, D, N, X, ldx, strideX, noise_kind, s, strides, prior_kind,
                          mw, stridemw, Lw, ldl, strideLw, mean, stridemean, var, stridevar, info):
        fn = getattr(self.lib, f"blr_marginals_batched_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, N, _ptr(X), ldx, strideX, noise_kind, _ptr(s), strides,
                             prior_kind, _ptr(mw), stridemw, _ptr(Lw), ldl, strideLw, _ptr(mean), stridemean,
                             _ptr(var), stridevar, _ptr(info)))

    def marginals_multi_batched(self, dtype, memspace, layout, B, D, N, S, X, ldx, strideX, noise_kind, s, strides, prior_kind,
                                M, ldm, strideM, Lw, ldl, strideLw, mean, ldmean, stridemean, var, stridevar, info):
        """S mean columns (M: D x S per regressor, as blr_posterior_multi_batched_* writes mw_post) and one variance per input
        for B regressors in one call; include/blr_mi355x.h blr_marginals_multi_batched_* (one status per regressor in info)."""
        fn = getattr(self.lib, f"blr_marginals_multi_batched_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, N, S, _ptr(X), ldx, strideX, noise_kind, _ptr(s), strides,
                             prior_kind, _ptr(M), ldm, strideM, _ptr(Lw), ldl, strideLw, _ptr(mean), ldmean, stridemean,
                             _ptr(var), stridevar, _ptr(info)))

    def rand(self, dtype, memspace, layout, D, N, S, X, ldx, noise_kind, s, prior_kind, mw, Lw, ldl, Z1, ldz1, Z2, ldz2,
             Y, ldy):
        fn = getattr(self.lib, f"blr_rand_{suffix(dtype)}")
        rc = self.check(fn(self._h, memspace, layout, D, N, S, _ptr(X), ldx, noise_kind, _ptr(s), prior_kind, _ptr(mw),
                           _ptr(Lw), ldl, _ptr(Z1), ldz1, _ptr(Z2), ldz2, _ptr(Y), ldy))
        if rc > 0:
            raise PosDefException(rc)
        return rc

    def rand_batched(self, dtype, memspace, layout, B, D, N, S, X, ldx, strideX, noise_kind, s, strides, prior_kind, mw, stridemw,
                     Lw, ldl, strideLw, Z1, ldz1, strideZ1, Z2, ldz2, strideZ2, W, ldw, strideW, Y, ldy, strideY, info):
        """Draws from B regressors in one call; include/blr_mi355x.h blr_rand_batched_* (per-regressor status in info)."""
        fn = getattr(self.lib, f"blr_rand_batched_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, N, S, _ptr(X), ldx, strideX, noise_kind, _ptr(s), strides, prior_kind,
                             _ptr(mw), stridemw, _ptr(Lw), ldl, strideLw, _ptr(Z1), ldz1, strideZ1, _ptr(Z2), ldz2, strideZ2,
                             _ptr(W), ldw, strideW, _ptr(Y), ldy, strideY, _ptr(info)))

    def rand_multi_batched(self, dtype, memspace, layout, B, D, N, S, R, X, ldx, strideX, noise_kind, s, strides, prior_kind, M, ldm,
                           strideM, Lw, ldl, strideLw, Z1, ldz1, strideZ1, Z2, ldz2, strideZ2, W, ldw, strideW, Y, ldy, strideY, info):
        """R draws from each of the S column posteriors (M: D x S per regressor, one shared factor) of B regressors in one call, draw
        j = c R + r; include/blr_mi355x.h blr_rand_multi_batched_* (per-regressor status in info)."""
        fn = getattr(self.lib, f"blr_rand_multi_batched_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, N, S, R, _ptr(X), ldx, strideX, noise_kind, _ptr(s), strides, prior_kind,
                             _ptr(M), ldm, strideM, _ptr(Lw), ldl, strideLw, _ptr(Z1), ldz1, strideZ1, _ptr(Z2), ldz2, strideZ2,
                             _ptr(W), ldw, strideW, _ptr(Y), ldy, strideY, _ptr(info)))

    def apply_weights(self, dtype, memspace, layout, D, N, S, X, ldx, W, ldw, Y, ldy):
        """Y (N x S) = X'W for S given weight vectors; include/blr_mi355x.h blr_apply_weights_*."""
        fn = getattr(self.lib, f"blr_apply_weights_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, D, N, S, _ptr(X), ldx, _ptr(W), ldw, _ptr(Y), ldy))

    def sample_weights(self, dtype, memspace, D, S, prior_kind, mw, Lw, ldl, Z, ldz, W, ldw):
        fn = getattr(self.lib, f"blr_sample_weights_{suffix(dtype)}")
        rc = self.check(fn(self._h, memspace, D, S, prior_kind, _ptr(mw), _ptr(Lw), ldl, _ptr(Z), ldz, _ptr(W), ldw))
        if rc > 0:
            raise PosDefException(rc)
        return rc

    def rff_features(self, dtype, memspace, Din, D, N, Xin, ldxin, Omega, ldo, phase, scale, Phi, ldphi):
        fn = getattr(self.lib, f"blr_rff_features_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, Din, D, N, _ptr(Xin), ldxin, _ptr(Omega), ldo, _ptr(phase), float(scale),
                             _ptr(Phi), ldphi))

    def posterior_rff(self, dtype, memspace, Din, D, N, Xin, ldxin, Omega, ldo, phase, scale, y, noise_kind, s, prior_kind,
                      mw, Lw, ldl, mw_post, T_post, ldt, Lw_post, ldlp, logpdf, info):
        fn = getattr(self.lib, f"blr_posterior_rff_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, Din, D, N, _ptr(Xin), ldxin, _ptr(Omega), ldo, _ptr(phase), float(scale),
                             _ptr(y), noise_kind, _ptr(s), prior_kind, _ptr(mw), _ptr(Lw), ldl, _ptr(mw_post), _ptr(T_post),
                             ldt, _ptr(Lw_post), ldlp, _ptr(logpdf), _ptr(info)))

    def posterior_dense_noise(self, dtype, memspace, layout, D, N, X, ldx, y, Sy, ldsy, prior_kind, mw, Lw, ldl, mw_post, T_post, ldt,
                              Lw_post, ldlp, logpdf, info):
        fn = getattr(self.lib, f"blr_posterior_dense_noise_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, D, N, _ptr(X), ldx, _ptr(y), _ptr(Sy), ldsy, prior_kind, _ptr(mw), _ptr(Lw), ldl,
                             _ptr(mw_post), _ptr(T_post), ldt, _ptr(Lw_post), ldlp, _ptr(logpdf), _ptr(info)))

    def mean_and_cov(self, dtype, memspace, layout, D, N, X, ldx, noise_kind, s, lds, prior_kind, mw, Lw, ldl, mean, Cov, ldc, info):
        fn = getattr(self.lib, f"blr_mean_and_cov_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, D, N, _ptr(X), ldx, noise_kind, _ptr(s), lds, prior_kind, _ptr(mw), _ptr(Lw), ldl,
                             _ptr(mean), _ptr(Cov), ldc, _ptr(info)))

    def mean_and_cov_batched(self, dtype, memspace, layout, B, D, N, X, ldx, strideX, noise_kind, s, lds, strides, prior_kind, mw, stridemw,
                             Lw, ldl, strideLw, mean, stridemean, Cov, ldc, strideC, info):
        """Mean (may be None) and the full N x N predictive covariance (may be None) of B regressors in one call;
        include/blr_mi355x.h blr_mean_and_cov_batched_* (one status per regressor in info)."""
        fn = getattr(self.lib, f"blr_mean_and_cov_batched_{suffix(dtype)}")
        return self.check(fn(self._h, memspace, layout, B, D, N, _ptr(X), ldx, strideX, noise_kind, _ptr(s), lds, strides, prior_kind,
                             _ptr(mw), stridemw, _ptr(Lw), ldl, strideLw, _ptr(mean), stridemean, _ptr(Cov), ldc, strideC, _ptr(info)))

    def rand_dense_noise(self, dtype, memspace, layout, D, N, S, X, ldx, Sy, ldsy, prior_kind, mw, Lw, ldl, Z1, ldz1, Z2, ldz2, Y, ldy):
        fn = getattr(self.lib, f"blr_rand_dense_noise_{suffix(dtype)}")
        rc = self.check(fn(self._h, memspace, layout, D, N, S, _ptr(X), ldx, _ptr(Sy), ldsy, prior_kind, _ptr(mw), _ptr(Lw), ldl,
                           _ptr(Z1), ldz1, _ptr(Z2), ldz2, _ptr(Y), ldy))
        if rc > 0:
            raise PosDefException(rc)
        return rc

    # -- RCCL called directly (one rank per handle) ------------------------------------------------------------------
    @staticmethod
    def comm_unique_id():
        """128 opaque bytes (rank 0 calls this and ships them to the other ranks)."""
        buf = C.create_string_buffer(128)
        rc = load_library().blr_comm_unique_id(C.cast(buf, _vp))
        if rc != 0:
            raise BLRError(rc, "blr_comm_unique_id failed (librccl missing?)")
        return buf.raw

    def comm_init(self, nranks, rank, unique_id):
        buf = C.create_string_buffer(bytes(unique_id), 128)
        return self.check(self.lib.blr_comm_init(self._h, int(nranks), int(rank), C.cast(buf, _vp)))

    def comm_destroy(self):
        return self.check(self.lib.blr_comm_destroy(self._h))

    def comm_size(self):
        return self.lib.blr_comm_size(self._h)

    def comm_rank(self):
        return self.lib.blr_comm_rank(self._h)

    def logpdf_allgather_sum(self, count, logpdf_local, logpdf_all, total):
        return self.check(self.lib.blr_logpdf_allgather_sum(self._h, count, _ptr(logpdf_local), _ptr(logpdf_all), _ptr(total)))

    def allreduce_sum(self, is_f64, buf, count):
        return self.check(self.lib.blr_allreduce_sum(self._h, int(bool(is_f64)), _ptr(buf), count))

    def logpdf_sum(self, memspace, B, logpdf, total):
        return self.check(self.lib.blr_logpdf_sum(self._h, memspace, B, _ptr(logpdf), _ptr(total)))


_default = {}
_default_lock = threading.Lock()


def default_handle(device=0):
    """Process-wide handle per device (created on first use; raises without a GPU)."""
    with _default_lock:
        key = (os.getpid(), device)
        if key not in _default:
            _default[key] = Handle(device)
        return _default[key]
