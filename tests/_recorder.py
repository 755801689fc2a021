"""A stand-in for the library handle, shared by the CPU routing tests of the held-out predictives (test_kfold_cpu.py,
test_kfold_large_cpu.py, test_loo_multi_cpu.py) and by the transcript test of their Python front (test_heldout_front_cpu.py).

It keeps "device" memory as host byte arrays behind made-up pointers, records every entry point with its arguments (``calls``), and
fills every output of a call with a fixed pattern so that the unpacking goes through: output k of a scoring call holds
``(10, 100, 1000, 10000)[k] + arange(count)`` in its own element type over the whole buffer (mean = 10 + n, var = 100 + n for one
regressor), the outputs of a fit ``1 + arange`` and ``2 + arange``.  ``fail`` makes one call report a failed regressor.

``events`` is the same history in a form that can be compared between two versions of the front (``transcript()``): a pointer
argument becomes a token ["ptr", ordinal, bytes, hash of the content at call time] -- the ordinal counts first appearance as an
argument, not allocation order --, a host array ["host", dtype, shape, hash], an element type its name; ``memcpy_d2h`` is an event
of its own, allocations, frees and uploads are not (an upload shows in the hash of the buffer at the call that reads it)."""
import hashlib

import numpy as np

_BASE = 0x7F0000000000  # no size, stride or count is ever this large: an int argument that is a key of ``bufs`` is a pointer

# name in ``calls`` and, per entry point, where its outputs sit: [(argument index, element type or None for the call's own)], info
_FIT = {"posterior_batched": ("posterior", [(20, None), (22, None)], 29),
        "posterior_multi_batched": ("fit", [(22, None), (25, None)], 33)}
_SCORE = {"loo": ("loo", [(19, None), (21, None), (23, np.float64), (25, np.float64)], 26),
          "kfold": ("kfold", [(20, None), (22, None), (24, np.float64), (26, np.float64)], 27),
          "kfold_large": ("kfold_large", [(20, None), (22, None), (24, np.float64), (26, np.float64)], 27),
          "loo_multi_batched": ("loo_multi", [(22, None), (25, None), (27, np.float64), (30, np.float64)], 32),
          "kfold_multi_batched": ("kfold_multi", [(23, None), (26, None), (28, np.float64), (31, np.float64)], 33)}


def digest(a):
    """16 hex digits of the bytes of an array in its own memory order"""
    return hashlib.sha1(np.asarray(a).reshape(-1, order="A").view(np.uint8).tobytes()).hexdigest()[:16]


class Recorder:
    """stands in for the library handle: records the entry points and fills status and outputs so that the unpacking goes through"""

    def __init__(self):
        self.calls = []     # (name, args) as the routing tests read them
        self.events = []    # the normalised history
        self.bufs = {}      # live device memory: pointer -> bytes
        self.sizes = {}     # pointer -> the size that was asked for (0 is allowed)
        self.fail = None    # (name in ``calls``, which call of that name, regressor k, info value)
        self._allocs = 0
        self._ordinal = {}

    # device memory as host arrays, keyed by a made-up pointer that is never handed out twice
    def device_alloc(self, nbytes):
        self._allocs += 1
        ptr = _BASE + 4096 * self._allocs
        self.bufs[ptr] = np.zeros(max(int(nbytes), 1), dtype=np.uint8)
        self.sizes[ptr] = int(nbytes)
        return ptr

    def device_free(self, ptr):
        self.bufs.pop(ptr, None)

    def memcpy_h2d(self, dptr, host):
        raw = np.asarray(host).reshape(-1, order="A").view(np.uint8)
        self.bufs[dptr][:raw.size] = raw

    def memcpy_d2h(self, host, dptr):
        flat = host.reshape(-1, order="A").view(np.uint8)
        self.events.append(["memcpy_d2h", self._token(dptr), int(flat.size)])
        flat[...] = self.bufs[dptr][:flat.size]

    def _token(self, ptr):
        n = self._ordinal.setdefault(ptr, len(self._ordinal))
        return ["ptr", n, self.sizes[ptr], digest(self.bufs[ptr][:self.sizes[ptr]])]

    def _norm(self, a):
        if a is None or isinstance(a, (bool, str)):
            return a
        if isinstance(a, type):
            return np.dtype(a).name
        if isinstance(a, np.ndarray):
            return ["host", a.dtype.name, list(a.shape), digest(a)]
        if isinstance(a, (int, np.integer)):
            return self._token(int(a)) if int(a) in self.bufs else int(a)
        return float(a)

    def _fill(self, target, dtype, base):
        if target is None:
            return
        if isinstance(target, np.ndarray):  # a host-memspace call writes into the caller's array
            target.reshape(-1, order="A")[...] = base + np.arange(target.size)
        else:
            self.memcpy_h2d(target, (base + np.arange(self.sizes[target] // np.dtype(dtype).itemsize)).astype(dtype))

    def _entry(self, name, outs, info, bases, args):
        self.events.append([name, [self._norm(a) for a in args]])  # (the arguments as the library finds them: before it writes)
        nth = sum(1 for k, _ in self.calls if k == name)
        self.calls.append((name, args))
        for (i, dt), base in zip(outs, bases):
            self._fill(args[i], dt or args[0], base)
        if self.fail is not None and self.fail[:2] == (name, nth) and info is not None:
            status = np.zeros(self.sizes[args[info]] // 4, dtype=np.int32)
            status[self.fail[2]] = self.fail[3]
            self.memcpy_h2d(args[info], status)
        return 0

    def rff_features(self, *args):
        return self._entry("rff_features", [(11, None)], None, (0.5,), args)

    def transcript(self):
        return self.events


def _method(table, key, bases):
    name, outs, info = table[key]
    return lambda self, *args: self._entry(name, outs, info, bases, args)


for _key in _FIT:
    setattr(Recorder, _key, _method(_FIT, _key, (1.0, 2.0)))
for _key in _SCORE:
    setattr(Recorder, _key, _method(_SCORE, _key, (10.0, 100.0, 1000.0, 10000.0)))
