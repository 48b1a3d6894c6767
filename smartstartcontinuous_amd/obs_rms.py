"""normalize_observations: the running observation statistics of DDPG_editted (ddpg_editted.py:14-18, 100-109).

The statistics object of the reference is baselines 0.1.5 ``common/mpi_running_mean_std.RunningMeanStd`` (third-party,
restated in DESIGN section 5): f64 ``sum`` (starts at 0), ``sumsq`` (1e-2) and ``count`` (1e-2); ``update(x)`` adds
sum(x), sum(x^2) and len(x) in f64; the networks see, in fp32 (TF ``to_float``),

    mean = f32(sum / count),  std = sqrt(max(f32(sumsq / count) - mean * mean, 1e-2))
    x_hat = clip((x - mean) / std, -obs_clip, obs_clip)

On the device the three live in ONE f64 block ``[sum[D] | sumsq[D] | count]`` (baselines' own Allreduce vector layout),
which every kernel reads when it starts: HIP graphs and the overlapped loop stay valid while it changes.
"""
from __future__ import annotations

import ctypes

import numpy as np
import torch

from . import _ffi

RMS_EPSILON = 1e-2


def rms_initial(obs_dim):
    """The f64 block of a fresh RunningMeanStd: sum 0, sumsq 1e-2, count 1e-2."""
    b = np.zeros(2 * obs_dim + 1, np.float64)
    b[obs_dim:] = RMS_EPSILON
    return b


def mean_std_f32(block, obs_dim=None):
    """The fp32 mean / std the networks use, from a host copy of the f64 block (numpy float32 arithmetic: one rounding
    per operation, no fused multiply-add -- the kernels' derivation)."""
    b = np.asarray(block, np.float64)
    d = (b.size - 1) // 2 if obs_dim is None else int(obs_dim)
    cnt = b[2 * d]
    mean = (b[:d] / cnt).astype(np.float32)
    sq = (b[d:2 * d] / cnt).astype(np.float32)
    var = sq - mean * mean                                    # float32 multiply, then float32 subtract
    std = np.sqrt(np.maximum(var, np.float32(RMS_EPSILON)))
    return mean, std.astype(np.float32)


def normalize_f32(x, block, obs_clip):
    """x_hat = clip((x - mean) / std, -obs_clip, obs_clip) in fp32 (numpy), for x [..., obs_dim]."""
    mean, std = mean_std_f32(block)
    xh = (np.asarray(x, np.float32) - mean) / std
    if obs_clip > 0:
        xh = np.clip(xh, np.float32(-obs_clip), np.float32(obs_clip))
    return xh.astype(np.float32)


class ObsRms:
    """The device block plus its update entry points (ssc_obs_rms_update / ssc_obs_rms_update_rows)."""

    def __init__(self, obs_dim, device="cuda"):
        self.obs_dim = int(obs_dim)
        if not 1 <= self.obs_dim <= _ffi.SSC_MAX_STATE:
            raise ValueError(f"obs_dim {obs_dim} out of range")
        self.device = torch.device(device)
        self.lib = _ffi.lib()
        self.block = torch.as_tensor(rms_initial(self.obs_dim), device=self.device)
        nbytes = int(self.lib.ssc_obs_rms_update_workspace_bytes(self.obs_dim))
        self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)

    def update_chunk(self, chunk, k0=0, K=None):
        """RunningMeanStd.update with the obs0 of steps [k0, K) of a TransitionChunk (every env)."""
        K = chunk.K if K is None else int(K)
        log = chunk.as_struct()
        with torch.cuda.device(self.device):
            _ffi.check(self.lib.ssc_obs_rms_update(self.obs_dim, ctypes.byref(log), int(k0), K, chunk.N,
                                                   _ffi.ptr(self.block), _ffi.ptr(self._ws), self._ws.numel(),
                                                   _ffi.stream(self.device)))

    def update_rows(self, x):
        """RunningMeanStd.update with the rows of x [m, obs_dim] (a host array or a tensor)."""
        t = torch.as_tensor(x, dtype=torch.float32, device=self.device).reshape(-1, self.obs_dim).contiguous()
        with torch.cuda.device(self.device):
            _ffi.check(self.lib.ssc_obs_rms_update_rows(self.obs_dim, t.shape[0], _ffi.ptr(t), _ffi.ptr(self.block),
                                                        _ffi.ptr(self._ws), self._ws.numel(), _ffi.stream(self.device)))

    def mean_std(self):
        """Host fp32 (mean, std): the values the kernels derive from the block."""
        return mean_std_f32(self.block.cpu().numpy(), self.obs_dim)

    def mean_std_device(self):
        """(mean, std) as fp32 DEVICE tensors [obs_dim], formed on the current stream without a host read, one tensor op
        per rounding of the kernels' derivation (f64 divide, round to fp32, fp32 multiply, subtract, max, square root)."""
        d, b = self.obs_dim, self.block
        cnt = b[2 * d]
        mean = (b[:d] / cnt).to(torch.float32)
        sq = (b[d:2 * d] / cnt).to(torch.float32)
        var = sq - mean * mean
        return mean, torch.sqrt(torch.clamp_min(var, RMS_EPSILON))

    def snapshot_into(self, other):
        """Stream-ordered copy of the block into ``other`` (an ObsRms or a tensor of the same shape)."""
        dst = other.block if isinstance(other, ObsRms) else other
        dst.copy_(self.block)
        return other


class ObsRmsGroup:
    """P :class:`ObsRms` blocks updated by TWO launches for all of them (``ssc_obs_rms_update_many``) instead of two each:
    every block ends up bit for bit as after ``rms.update_chunk`` one by one (each block's rows are partitioned and summed
    exactly as its own call does it).  Blocks of different obs_dim, or two entries on one block, update one by one;
    ``fused`` tells which way the last call went.  The descriptors are rebuilt only when a pointer, a shape, the step range
    or the stream changes."""

    def __init__(self, blocks):
        self.blocks = list(blocks)
        if not self.blocks:
            raise ValueError("a group needs at least one statistics block")
        self.device, self.lib = self.blocks[0].device, self.blocks[0].lib
        self.fused = None
        self._sig = self._items = None

    def update_chunks(self, chunks, k0=0, K=None):
        """``blocks[p].update_chunk(chunks[p], k0[p], K[p])`` for every p; ``k0`` / ``K``: one value or one per block."""
        bs, chunks = self.blocks, list(chunks)
        k0s = [int(k0)] * len(bs) if isinstance(k0, int) else [int(x) for x in k0]
        Ks = [K] * len(bs) if K is None or isinstance(K, int) else list(K)
        Ks = [c.K if k is None else int(k) for c, k in zip(chunks, Ks)]
        sig = (torch.cuda.current_stream(self.device).cuda_stream, tuple(k0s), tuple(Ks),
               tuple((b.block.data_ptr(), b._ws.data_ptr(), c.obs.data_ptr(), c.obs.stride(0), c.act.stride(0), c.N)
                     for b, c in zip(bs, chunks)))
        if sig != self._sig:
            from .population import DeviceItems
            self._sig, self._items = sig, None
            self.fused = (all(b.obs_dim == bs[0].obs_dim and b.device == self.device for b in bs) and bs[0].obs_dim <= _ffi.SSC_MAX_OBS
                          and len({b.block.data_ptr() for b in bs}) == len(bs) and len(bs) <= 65535)
            if self.fused:
                items = DeviceItems(_ffi.ObsRmsItem, len(bs), self.device)
                for it, b, c, a, e in zip(items.items, bs, chunks, k0s, Ks):
                    it.log, it.k0, it.K, it.n = c.as_struct(), a, e, c.N
                    it.d_rms, it.d_workspace, it.workspace_bytes = b.block.data_ptr(), b._ws.data_ptr(), b._ws.numel()
                items.upload()
                self._items = items
        if not self.fused:
            for b, c, a, e in zip(bs, chunks, k0s, Ks):
                b.update_chunk(c, a, e)
            return
        with torch.cuda.device(self.device):
            _ffi.check(self.lib.ssc_obs_rms_update_many(bs[0].obs_dim, self._items.h_ptr, self._items.d_ptr, len(bs),
                                                        _ffi.stream(self.device)))
