"""Launch descriptors of the population entry points (``ssc_rollout_many``, ``ssc_replay_append_many``,
``ssc_decay_schedule_many``, ``ssc_obs_rms_update_many``, ``ssc_ddpg_eval_rollout_many``, ``ssc_ddpg_stats_many``,
``ssc_param_noise_cycle_many``, the ``DDPGPopulation`` learner).

Each of those calls takes a host array that the library validates and the caller's device copy of the same bytes.
``DeviceItems`` is that pair for one ctypes struct: pinned host memory, a non-blocking copy, and an event that guards the
pinned bytes against being rewritten while an upload still reads them.  ``PairCursors`` is the small per-chunk array
(``ssc_pair_cursor``: ``step0`` for the rollout, ``replay_start`` for the append) that a steady-state chunk uploads and
nothing else; ``IndexDraw`` is the same for the sampling keys of ``ssc_replay_sample_many``.
"""
from __future__ import annotations

import ctypes

import torch

from . import _ffi


class DeviceItems:
    """``n`` structs of ``ctype`` in pinned host memory (``items``, a ctypes array over it) and their device copy."""

    def __init__(self, ctype, n, device):
        self.device = torch.device(device)
        self.n = int(n)
        nbytes = ctypes.sizeof(ctype) * self.n
        self.host = torch.zeros(nbytes, dtype=torch.uint8).pin_memory()
        with torch.cuda.device(self.device):
            self.dev = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
            self._event = torch.cuda.Event()
        self.items = (ctype * self.n).from_address(self.host.data_ptr())
        self._pending = False

    def wait(self):
        """Before the pinned bytes are rewritten: the last upload has read them."""
        if self._pending:
            self._event.synchronize()
            self._pending = False

    def upload(self):
        """Stream-ordered copy to the device (current stream); the kernels queued behind it see these bytes."""
        with torch.cuda.device(self.device):
            self.dev.copy_(self.host, non_blocking=True)
            self._event.record()
        self._pending = True

    @property
    def h_ptr(self):
        return self.host.data_ptr()

    @property
    def d_ptr(self):
        return self.dev.data_ptr()


class PairCursors(DeviceItems):
    """What changes with every chunk, 16 bytes per pair: ``step0`` (``ssc_rollout_many``) and ``replay_start``
    (``ssc_replay_append_many``).  ``stage`` writes the host values, ``upload`` sends them; a loop that knows both before
    the rollout uploads once per chunk and hands the same object to both wrappers."""

    def __init__(self, n, device):
        super().__init__(_ffi.PairCursor, n, device)

    def stage(self, step0=None, replay_start=None):
        self.wait()
        if step0 is not None:
            for c, v in zip(self.items, step0):
                c.step0 = int(v)
        if replay_start is not None:
            for c, v in zip(self.items, replay_start):
                c.replay_start = int(v)
        return self

    def step0(self):
        return [int(c.step0) for c in self.items]

    def replay_start(self):
        return [int(c.replay_start) for c in self.items]


class IndexDraw:
    """Batch indices of up to ``n`` rings in one ``ssc_replay_sample_many``: the keys (``keys``, a ``DeviceItems`` of
    ``ReplaySampleKey``) and ``idx`` int32 [n, n_max, B]; ring j's batches are row j, its consumer reads its first ones."""

    def __init__(self, n, n_max, B, device):
        self.keys = DeviceItems(_ffi.ReplaySampleKey, n, device)
        self.n_max, self.B = int(n_max), int(B)
        self.idx = torch.empty((self.keys.n, self.n_max, self.B), dtype=torch.int32, device=self.keys.device)

    def draw(self, keys):
        """upload ``keys`` ((seed, counter0, size) of rings 0 .. len(keys) - 1) and draw their rows on the current stream"""
        k = self.keys
        k.wait()
        for it, key in zip(k.items, keys):
            it.seed, it.counter0, it.size = key
        k.upload()
        with torch.cuda.device(k.device):
            _ffi.check(_ffi.lib().ssc_replay_sample_many(k.h_ptr, k.d_ptr, len(keys), self.n_max, self.B, _ffi.ptr(self.idx),
                                                         _ffi.stream(k.device)))


def served(rc):
    """Does a validation-only call (nothing to launch) say the population is served by the one launch?  SSC_EINVAL /
    SSC_EUNSUPPORTED: no -- the caller runs the per-pair calls; anything else is an error."""
    if rc == _ffi.SSC_OK:
        return True
    if rc in (_ffi.SSC_EINVAL, _ffi.SSC_EUNSUPPORTED):
        return False
    _ffi.check(rc)
    return False
