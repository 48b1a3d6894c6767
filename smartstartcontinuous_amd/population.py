"""Launch descriptors of the population entry points (``ssc_rollout_many``, ``ssc_replay_append_many``,
``ssc_decay_schedule_many``, ``ssc_obs_rms_update_many``, ``ssc_ddpg_eval_rollout_many``, ``ssc_ddpg_stats_many``,
``ssc_param_noise_cycle_many``).

Each of those calls takes a host array that the library validates and the caller's device copy of the same bytes.
``DeviceItems`` is that pair for one ctypes struct; ``PairCursors`` is the small per-chunk array (``ssc_pair_cursor``:
``step0`` for the rollout, ``replay_start`` for the append) that a steady-state chunk uploads and nothing else.
``agents.DDPGPopulation._prepare`` is the model: pinned host memory, a non-blocking copy, and an event that guards the
pinned bytes against being rewritten while an upload still reads them.
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


def served(rc):
    """Does a validation-only call (nothing to launch) say the population is served by the one launch?  SSC_EINVAL /
    SSC_EUNSUPPORTED: no -- the caller runs the per-pair calls; anything else is an error."""
    if rc == _ffi.SSC_OK:
        return True
    if rc in (_ffi.SSC_EINVAL, _ffi.SSC_EUNSUPPORTED):
        return False
    _ffi.check(rc)
    return False
