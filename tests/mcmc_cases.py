"""Shared by tests/test_mcmc_chains.py and tests/test_batch_slabs.py: the Philox position the next launch takes, the accept
uniforms of nf_metropolis_chains restated with the oracle's Philox, the documented rule step by step in numpy double, and
one launch of the kernel on host arrays."""
import math

import numpy as np
import torch

from normflow__amd import _hip
from oracle import nf_oracle as O

DEV = torch.device("cuda", 0)
CHAIN_DOMAIN = 0x6E666368          # NF_PHILOX_CHAIN_DOMAIN


def position():
    """(seed, kernel offset) the next Philox launch will use (the host bridge reads torch's CUDA generator)."""
    gen = torch.cuda.default_generators[0]
    return gen.initial_seed(), gen.get_offset() // 4


def log_uniforms(seed, offset, n):
    """log u_r of nf_metropolis_chains: counter (lo32 r, hi32 r, lo32 offset, hi32 offset), key (lo32 seed, hi32 seed ^
    chain domain), u = ((r0 << 21 ^ r1 >> 11) + 1) 2^-53 in (0, 1]."""
    r = np.arange(n, dtype=np.uint64)
    ctr = np.stack([r & np.uint64(0xFFFFFFFF), r >> np.uint64(32), np.full_like(r, offset & 0xFFFFFFFF),
                    np.full_like(r, (offset >> 32) & 0xFFFFFFFF)], axis=-1).astype(np.uint32)
    key = np.broadcast_to(np.array([seed & 0xFFFFFFFF, ((seed >> 32) & 0xFFFFFFFF) ^ CHAIN_DOMAIN], dtype=np.uint32),
                          (n, 2))
    w = O.philox4x32_10(ctr, key).astype(np.uint64)
    a = (w[:, 0] << np.uint64(21)) ^ (w[:, 1] >> np.uint64(11))
    return np.log((a.astype(np.float64) + 1.0) * 2.0 ** -53)


def scan(logq, logp, ref, ref_lq, ref_lp, logu, S, C, fresh):
    """The documented rule in numpy double, step by step: flags, keep, selected log q / log p, final state and the
    smallest |margin| of a decision that was not forced."""
    d = (logq.astype(np.float64) - logp.astype(np.float64)).reshape(S, C)
    logu = logu.reshape(S, C)
    lq, lp = logq.reshape(S, C), logp.reshape(S, C)
    ref, cur_lq, cur_lp, last = ref.copy(), ref_lq.copy(), ref_lp.copy(), np.arange(C, dtype=np.int64)
    flags, keep = np.empty((S, C), dtype=bool), np.empty((S, C), dtype=np.int64)
    sel_q, sel_p = np.empty_like(lq), np.empty_like(lp)
    tight = math.inf
    for s in range(S):
        if fresh and s == 0:
            ok = np.ones(C, dtype=bool)
        else:
            with np.errstate(invalid='ignore'):
                margin = logu[s] - (ref - d[s])
            ok = margin < 0
            finite = np.isfinite(margin)
            if finite.any():
                tight = min(tight, np.abs(margin[finite]).min())
        ref = np.where(ok, d[s], ref)
        cur_lq, cur_lp = np.where(ok, lq[s], cur_lq), np.where(ok, lp[s], cur_lp)
        last = np.where(ok, s * C + np.arange(C), last)
        flags[s], keep[s], sel_q[s], sel_p[s] = ok, last, cur_lq, cur_lp
    return flags.ravel(), keep.ravel(), sel_q.ravel(), sel_p.ravel(), ref, cur_lq, cur_lp, tight


def run_chains(logq, logp, ref, ref_lq, ref_lp, C, fresh, dtype):
    """One launch on host arrays: (flags, keep, sel_q, sel_p, ref, ref_lq, ref_lp) as numpy, and the position it used."""
    dev = lambda a, dt: torch.as_tensor(a, dtype=dt, device="cpu").to(DEV).contiguous()
    B = logq.shape[0]
    t = dict(logq=dev(logq, dtype), logp=dev(logp, dtype), ref=dev(ref, torch.float64), rq=dev(ref_lq, dtype),
             rp=dev(ref_lp, dtype), flags=torch.full((B,), 7, dtype=torch.uint8, device=DEV),
             keep=torch.full((B,), -1, dtype=torch.int64, device=DEV),
             sq=torch.full((B,), float('nan'), dtype=dtype, device=DEV),
             sp=torch.full((B,), float('nan'), dtype=dtype, device=DEV))
    pos = position()
    _hip.metropolis_chains(t['logq'], t['logp'], t['ref'], t['rq'], t['rp'], t['flags'], t['keep'], t['sq'], t['sp'], C,
                           fresh=fresh)
    torch.cuda.synchronize()
    assert position() == (pos[0], pos[1] + 1)                     # one launch consumes one offset
    return [t[k].cpu().numpy() for k in ('flags', 'keep', 'sq', 'sp', 'ref', 'rq', 'rp')], pos
