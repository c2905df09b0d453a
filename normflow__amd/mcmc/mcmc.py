"""Metropolis sampling on top of the flow (reference: src/mcmc/mcmc.py).

`MCMCSampler` (independence Metropolis): the proposals come from `posterior.sample__`, i.e. from the HIP path.  By default
the accept/reject is the reference's host code (one chain over the batch, `np.random` uniforms).  A chain is serial, but
chains are independent: with `n_chains=C` on a HIP device the decisions of C chains are taken by one launch of
nf_metropolis_chains and the rejected rows are overwritten in place by nf_metropolis_select (nf_mcmc.hip), with one read
of the flags per call.  `BlockedMCMCSampler` redraws one block of the prior-side field at a
time; on a HIP device it runs C independent chains batched through the flow, with proposal, accept/reject and restore
on the GPU (nf_mcmc.hip)."""
import copy

import numpy as np
import torch

from .. import _hip
from ..lib.stats import Resampler, estimate_logz, fmt_val_err

seize = lambda t: t.detach().cpu().numpy()


class Metropolis:
    @staticmethod
    @torch.no_grad()
    def calc_accept_status(logqp, logqp_ref=None):
        """accept[i] = log u_i < logqp_ref - logqp[i], ref updated on accept (mcmc.py:304-317)."""
        logqp = np.asarray(logqp)
        ref = logqp[0] if logqp_ref is None else logqp_ref
        logu = np.log(np.random.rand(logqp.shape[0]))
        status = np.empty(len(logqp), dtype=bool)
        for i, cur in enumerate(logqp):
            status[i] = logu[i] < ref - cur
            if status[i]:
                ref = cur
        return status

    @staticmethod
    def calc_accept_indices(accept_seq):
        """Index of the configuration kept at each chain position (mcmc.py:319-328)."""
        idx = np.arange(len(accept_seq))
        last = 0
        for i, ok in enumerate(accept_seq):
            if ok:
                last = i
            else:
                idx[i] = last
        return idx

    @staticmethod
    def calc_accept_count(accept_seq):
        pos = np.where(accept_seq)[0]
        return pos[1:] - pos[:-1]

    @staticmethod
    def calc_tau_rejections_prob(accept_seq, max_tau=100):
        """p[tau] = fraction of positions i with tau + 1 rejections in a row from i on (mcmc.py:338-351)."""
        rej = ~np.asarray(accept_seq, dtype=bool)
        p_tau = np.zeros(max_tau)
        run = rej
        p_tau[0] = np.mean(run)
        for tau in range(1, max_tau):
            run = run[:-1] & rej[tau:]
            p_tau[tau] = np.mean(run)
        return p_tau


class ModifiedMetropolis(Metropolis):
    """Metropolis with an extra Gaussian penalty tau (logqp_ref - logqp)^2 on the log acceptance (mcmc.py:354-375)."""

    @staticmethod
    @torch.no_grad()
    def calc_accept_status(logqp, logqp_ref=None, tau=0):
        logqp = np.asarray(logqp)
        ref = logqp[0] if logqp_ref is None else logqp_ref
        logu = np.log(np.random.rand(logqp.shape[0]))
        status = np.empty(len(logqp), dtype=bool)
        for i, cur in enumerate(logqp):
            d = ref - cur
            status[i] = logu[i] < -(tau * d ** 2 + (-d if d < 0 else 0))
            if status[i]:
                ref = cur
        return status


class MCMCHistory:
    _KEYS = ('logq', 'logp', 'raw_logq', 'raw_logp', 'accept_seq', 'accept_ind', 'accept_rate')

    def __init__(self):
        self.reset_history()

    def reset_history(self):
        for k in self._KEYS:
            setattr(self, k, [])

    def bookkeeping(self, **items):
        for k, v in items.items():
            if v is None:
                continue
            if k in ('logq', 'logp'):
                v = seize(v)
            elif k in ('raw_logq', 'raw_logp'):
                v = copy.copy(seize(v))
            getattr(self, k).append(v)

    @property
    def logqp(self):
        return [q - p for q, p in zip(self.logq, self.logp)]

    @property
    def raw_logqp(self):
        return [q - p for q, p in zip(self.raw_logq, self.raw_logp)]

    def report_summary(self, since=0, asstr=False):
        fmt = (lambda m, s: fmt_val_err(m, s, err_digits=2)) if asstr else (lambda m, s: (m, s))
        logqp = torch.tensor(self.logq[-1] - self.logp[-1])
        rate = torch.tensor(self.accept_rate)
        ms = lambda t: (t.mean().item(), t.std().item())
        return {'logqp': fmt(*ms(logqp)), 'logz': fmt(*estimate_logz(logqp)), 'accept_rate': fmt(*ms(rate))}


class MCMCSampler:
    """Draw proposals from the flow, keep/repeat them by Metropolis (mcmc.py:15-128).

    MI355X-side extension (no counterpart in the reference), like `BlockedMCMCSampler(n_chains=)`: `n_chains=C` runs C
    independent chains on one batch of proposals; proposal row r is step r // C of chain r % C, output row r the state of
    chain r % C after step r // C, and `_ref` keeps every chain's last state, so the next call continues all C chains
    (C = 1 keeps the reference's `_ref` shapes: calls with n_chains=None and n_chains=1 continue each other).  On a HIP
    device with the kernel prior (NormalPrior with torch_rng=False) the accept/reject is nf_metropolis_chains and
    nf_metropolis_select: no host loop, no gather, one device-to-host read (the flags) per call; its uniforms are that
    kernel's stream (include/normflow_hip.h), keyed by torch's CUDA generator.  On CPU tensors, or with torch_rng=True,
    the same rule runs on the host with `np.random` uniforms.  `n_chains=None` (the default) is the reference's code."""

    def __init__(self, model):
        self._model = model
        self.history = MCMCHistory()
        self._ref = dict(sample=None, logq=None, logp=None, logqp=None)

    @torch.no_grad()
    def sample(self, batch_size=1, **kwargs):
        return self.sample__(batch_size=batch_size, **kwargs)[0]

    @torch.no_grad()
    def sample_(self, batch_size=1, **kwargs):
        return self.sample__(batch_size=batch_size, **kwargs)[:2]

    @torch.no_grad()
    def sample__(self, batch_size=1, bookkeeping=False, n_chains=None):
        if n_chains is not None:
            n_chains = int(n_chains)
            if n_chains < 1 or batch_size < 1 or batch_size % n_chains != 0:
                raise ValueError(f"batch_size ({batch_size}) must be a positive multiple of n_chains ({n_chains})")
        else:
            self._ref_for_host_chain()
        y, logq, logp = self._model.posterior.sample__(batch_size=batch_size)
        if bookkeeping:
            self.history.bookkeeping(raw_logq=logq, raw_logp=logp)
        if n_chains is None:
            y, logq, logp = self._accept_reject_step(y, logq, logp, bookkeeping=bookkeeping)
        else:
            y, logq, logp = self._accept_reject_chains(y, logq, logp, n_chains, bookkeeping=bookkeeping)
        if bookkeeping:
            self.history.bookkeeping(logq=logq, logp=logp)
        return y, logq, logp

    @torch.no_grad()
    def _accept_reject_step(self, y, logq, logp, bookkeeping=False):
        ref = self._ref
        accept = Metropolis.calc_accept_status(seize(logq - logp), ref['logqp'])
        if not accept[0]:
            y[0], logq[0], logp[0] = ref['sample'], ref['logq'], ref['logp']
        keep = Metropolis.calc_accept_indices(accept)
        keep_t = torch.as_tensor(keep, dtype=torch.long, device=y.device)
        y, logq, logp = (t.index_select(0, keep_t) for t in (y, logq, logp))
        ref.update(sample=y[-1], logq=logq[-1].item(), logp=logp[-1].item())
        ref['logqp'] = ref['logq'] - ref['logp']
        self.history.bookkeeping(accept_rate=np.mean(accept))
        if bookkeeping:
            self.history.bookkeeping(accept_seq=accept, accept_ind=keep)
        return y, logq, logp

    # ---- n_chains=C: C independent chains on one batch of proposals
    def _on_device(self, y, logq):
        return (y.is_cuda and not getattr(self._model.prior, 'torch_rng', True)
                and logq.dtype in (torch.float32, torch.float64))

    def _stored_chains(self, n_chains):
        """True if `_ref` holds the state of n_chains chains (else the chains start fresh, with the blocked sampler's message)."""
        s = self._ref['sample']
        shape = tuple(self._model.prior.shape)
        want = shape if n_chains == 1 else (n_chains, *shape)
        if s is not None and self._ref['logqp'] is not None and tuple(s.shape) == want:
            return True
        print("Starting from scratch & setting logqp_ref to None")
        return False

    def _ref_for_host_chain(self):
        """Before the reference's single-chain code runs: a state left by a device call with n_chains=1 (0-dim device tensors)
        becomes the floats that code keeps; the state of several chains cannot continue one chain and is dropped."""
        ref = self._ref
        if ref['sample'] is None:
            return
        if tuple(ref['sample'].shape) != tuple(self._model.prior.shape):
            print("Starting from scratch & setting logqp_ref to None")
            ref.update(sample=None, logq=None, logp=None, logqp=None)
        elif torch.is_tensor(ref['logqp']):
            ref.update(logq=ref['logq'].item(), logp=ref['logp'].item())
            ref['logqp'] = ref['logq'] - ref['logp']

    def _store_chains(self, n_chains, sample, logq, logp, logqp):
        """`_ref` for the next call: (C, ...) tensors, or for one chain the reference's shapes (prior.shape and scalars)."""
        if n_chains == 1:
            sample, logq, logp, logqp = sample[0], logq[0], logp[0], logqp[0]
        self._ref.update(sample=sample, logq=logq, logp=logp, logqp=logqp)

    @torch.no_grad()
    def _accept_reject_chains(self, y, logq, logp, n_chains, bookkeeping=False):
        batch = y.shape[0]
        if logp.dtype != logq.dtype:
            logp = logp.to(logq.dtype)
        cont = self._stored_chains(n_chains)
        if self._on_device(y, logq):
            y, logq, logp, flags, keep = self._chains_device(y, logq, logp, n_chains, cont)
            accept = flags.cpu().numpy().astype(bool)             # the one device-to-host read of the call
            keep = keep.cpu().numpy() if bookkeeping else None
        else:
            y, logq, logp, accept, keep = self._chains_host(y, logq, logp, n_chains, cont)
        self.history.bookkeeping(accept_rate=np.mean(accept))
        if bookkeeping:
            shape = (batch,) if n_chains == 1 else (batch // n_chains, n_chains)
            self.history.bookkeeping(accept_seq=accept.reshape(shape), accept_ind=keep.reshape(shape))
        return y, logq, logp

    def _chains_device(self, y, logq, logp, n_chains, cont):
        """The two launches; nothing here copies to or from the host or synchronises when `_ref` holds device tensors."""
        C, dev, dt = n_chains, y.device, logq.dtype
        y, logq, logp = y.contiguous(), logq.contiguous(), logp.contiguous()
        ref = self._ref
        if cont:
            state = lambda v, t: torch.as_tensor(v, dtype=t).to(dev).reshape(C).contiguous()
            ref_s = ref['sample'].to(device=dev, dtype=y.dtype).contiguous()
            ref_q, ref_p, ref_qp = state(ref['logq'], dt), state(ref['logp'], dt), state(ref['logqp'], torch.float64)
        else:
            ref_s = None
            ref_q, ref_p = torch.empty(C, dtype=dt, device=dev), torch.empty(C, dtype=dt, device=dev)
            ref_qp = torch.empty(C, dtype=torch.float64, device=dev)
        flags = torch.empty(y.shape[0], dtype=torch.uint8, device=dev)
        keep = torch.empty(y.shape[0], dtype=torch.int64, device=dev)
        logq_sel, logp_sel = torch.empty_like(logq), torch.empty_like(logp)
        _hip.metropolis_chains(logq, logp, ref_qp, ref_q, ref_p, flags, keep, logq_sel, logp_sel, C, fresh=not cont)
        _hip.metropolis_select(y, ref_s, flags, keep, C)
        self._store_chains(C, y[-C:].clone(), ref_q, ref_p, ref_qp)
        return y, logq_sel, logp_sel, flags, keep

    def _chains_host(self, y, logq, logp, n_chains, cont):
        """The same rule on the host, vectorised over the chains: one np.random.rand(S, C), a loop over the S steps.  With
        one chain it consumes np.random as the reference's code does and returns what that code returns."""
        C, batch = n_chains, y.shape[0]
        S = batch // C
        d = seize(logq.double() - logp.double()).reshape(S, C)
        logu = np.log(np.random.rand(S, C))
        ref = self._ref
        if cont:
            cur = seize(torch.as_tensor(ref['logqp'], dtype=torch.float64)).reshape(C).copy()
        accept = np.empty((S, C), dtype=bool)
        keep = np.empty((S, C), dtype=np.int64)
        last = np.arange(C)
        for s in range(S):
            ok = logu[s] < cur - d[s] if (cont or s > 0) else np.ones(C, dtype=bool)
            cur = np.where(ok, d[s], cur) if (cont or s > 0) else d[s].copy()
            last = np.where(ok, s * C + np.arange(C), last)
            accept[s], keep[s] = ok, last
        held = ~accept[0]                           # chains that reject their first proposal hold the stored state in row c
        if held.any():
            rows = torch.as_tensor(np.flatnonzero(held), device=y.device)
            as_rows = lambda v, like: torch.as_tensor(v, dtype=like.dtype).to(like.device).reshape(C, *like.shape[1:])
            y[rows] = as_rows(ref['sample'], y)[rows]
            logq[rows] = as_rows(ref['logq'], logq)[rows]
            logp[rows] = as_rows(ref['logp'], logp)[rows]
        keep_t = torch.as_tensor(keep.ravel(), device=y.device)
        y, logq, logp = (t.index_select(0, keep_t) for t in (y, logq, logp))
        if C == 1:
            lq, lp = logq[-1].item(), logp[-1].item()
            self._ref.update(sample=y[-1].clone(), logq=lq, logp=lp, logqp=lq - lp)
        else:
            self._store_chains(C, y[-C:].clone(), logq[-C:].clone(), logp[-C:].clone(),
                               torch.as_tensor(cur, dtype=torch.float64, device=y.device))
        return y, logq, logp, accept.ravel(), keep.ravel()

    @torch.no_grad()
    def serial_sample_generator(self, n_samples, batch_size=16):
        for i in range(n_samples):
            j = i % batch_size
            if j == 0:
                y, logq, logp = self.sample__(batch_size)
            yield y[j].unsqueeze(0), logq[j].unsqueeze(0), logp[j].unsqueeze(0)

    @torch.no_grad()
    def calc_accept_rate(self, n_samples=1024, batch_size=None, n_resamples=10, method='shuffling'):
        if batch_size is None or batch_size > n_samples:
            batch_size = n_samples
        chunks = []
        for _ in range(int(np.ceil(n_samples / batch_size))):
            _, logq, logp = self._model.posterior.sample__(batch_size=batch_size)
            chunks.append(seize(logq - logp))
        return self.estimate_accept_rate(np.concatenate(chunks))

    @staticmethod
    @torch.no_grad()
    def estimate_accept_rate(logqp, n_resamples=10, method='shuffling'):
        if torch.is_tensor(logqp):
            logqp = seize(logqp)
        rate = lambda q: np.mean(Metropolis.calc_accept_status(q))
        return Resampler(method).eval(logqp, fn=rate, n_resamples=n_resamples)

    def log_prob(self, y, action_logz=0):
        return -self._model.action(y) - action_logz


class BlockedMCMCSampler(MCMCSampler):
    """Metropolis with block updates of the prior-side field x (mcmc.py:132-220): a sweep redraws the blocks of x one at a
    time from the prior, pushes x through the flow and accepts or rejects the new block by log u < logqp_ref - (logq - logp).

    With n_chains=1 it is the reference's sampler: the same start, `_ref` update, history keys and return shapes.
    MI355X-side extension (no counterpart in the reference), like `Posterior.graphed`: `n_chains=C` runs C independent
    chains at once; output row r is sweep r // C of chain r % C, and `_ref` keeps every chain's last configuration and
    logqp, so the next call continues all C chains.  On a HIP device with the kernel prior (NormalPrior with
    torch_rng=False) a block step is nf_block_propose, the flow and the action at batch C, and nf_block_accept: no host
    synchronisation per block, the accept flags collect on the device and are read once per `sample__`.  Its random
    streams are those kernels' (include/normflow_hip.h), keyed by torch's CUDA generator.  On CPU tensors, or with
    torch_rng=True, the reference's loop runs as written (torch's sampler, `np.random` uniforms)."""

    @torch.no_grad()
    def sample(self, batch_size=1, **kwargs):
        return self.sample__(batch_size=batch_size, **kwargs)[0]

    @torch.no_grad()
    def sample_(self, batch_size=1, **kwargs):
        return self.sample__(batch_size=batch_size, **kwargs)[:2]

    @torch.no_grad()
    def sample__(self, batch_size=1, n_blocks=1, bookkeeping=False, n_chains=1):
        """(cfgs, logq, logp) of batch_size samples: batch_size // n_chains sweeps of every chain."""
        prior = self._model.prior
        n_chains = int(n_chains)
        if n_chains < 1 or batch_size % n_chains != 0:
            raise ValueError(f"batch_size ({batch_size}) must be a positive multiple of n_chains ({n_chains})")
        block_len, n_blocks = self._block_len(n_blocks)
        x, logqp_ref = self._start(n_chains)
        prior.setup_blockupdater(block_len)

        n_sweeps = batch_size // n_chains
        cfgs = torch.empty((batch_size, *prior.shape), dtype=x.dtype, device=x.device)
        logq = torch.empty((batch_size,), dtype=x.dtype, device=x.device)
        logp = torch.empty((batch_size,), dtype=x.dtype, device=x.device)
        device = self._on_device(x)
        if device:
            ref_t = self._ref_tensor(logqp_ref, n_chains, x.device)
            flags = torch.empty((n_sweeps, n_blocks, n_chains), dtype=torch.uint8, device=x.device)
        else:
            accept_seq = np.empty((batch_size, n_blocks), dtype=bool)

        for s in range(n_sweeps):
            rows = slice(s * n_chains, (s + 1) * n_chains)
            if device:
                self._sweep_device(x, n_blocks, ref_t, flags[s], fresh=(logqp_ref is None and s == 0))
            else:
                acc, logqp_ref = self._sweep_host(x, n_blocks, logqp_ref)
                accept_seq[rows] = acc.reshape(n_chains, n_blocks)
            y, lq, lp = self._evaluate(x)
            cfgs[rows], logq[rows], logp[rows] = y, lq, lp
        if device:     # the one read of the flags per call
            accept_seq = flags.permute(0, 2, 1).reshape(batch_size, n_blocks).cpu().numpy().astype(bool)

        # update the '_ref' dictionary for the next round
        if n_chains == 1:
            self._ref['sample'] = y[-1]
            self._ref['logq'] = logq[-1].item()
            self._ref['logp'] = logp[-1].item()
            self._ref['logqp'] = (logq[-1] - logp[-1]).item()
        else:
            self._ref.update(sample=y, logq=lq, logp=lp, logqp=(lq - lp).to(torch.float64))

        self.history.bookkeeping(accept_rate=np.mean(accept_seq))  # always save
        if bookkeeping:
            self.history.bookkeeping(logq=logq, logp=logp)
            self.history.bookkeeping(accept_seq=accept_seq.ravel() if n_chains == 1 else accept_seq)
        return cfgs, logq, logp

    @torch.no_grad()
    def sweep(self, x, n_blocks=1, logqp_ref=None):
        """In-place sweeper over the n_blocks blocks of x (C, *shape): returns (accept_seq, logqp_ref), accept_seq of shape
        (n_blocks,) for one chain and (C, n_blocks) for C; logqp_ref None starts fresh chains (first block accepted)."""
        block_len, n_blocks = self._block_len(n_blocks)
        prior = self._model.prior
        bu = getattr(prior, 'blockupdater', None)
        if bu is None or bu.block_len != block_len:
            prior.setup_blockupdater(block_len)
        self._check_field(x)
        if not self._on_device(x):
            return self._sweep_host(x, n_blocks, logqp_ref)
        n = x.shape[0]
        ref_t = self._ref_tensor(logqp_ref, n, x.device)
        flags = torch.empty((n_blocks, n), dtype=torch.uint8, device=x.device)
        self._sweep_device(x, n_blocks, ref_t, flags, fresh=logqp_ref is None)
        acc = flags.t().cpu().numpy().astype(bool)
        if n == 1:
            return acc[0], ref_t.item()
        return acc, ref_t

    @torch.no_grad()
    def step(self, x, block_ind, logqp_ref, accept_out, force_accept=False):
        """One block step of C chains on the device, in place: nf_block_propose, the flow and the action at batch C, then
        nf_block_accept, which updates logqp_ref (C) float64 and writes the flags into accept_out (C) uint8."""
        prior, model = self._model.prior, self._model
        bu = prior.blockupdater
        bu(x, block_ind)
        y, logJ = model.net_(x)
        logq = (prior.log_prob(x) - logJ).to(x.dtype)
        logp = (-model.action(y)).to(x.dtype)
        _hip.block_accept(x, bu.backup_block, logq.contiguous(), logp.contiguous(), logqp_ref, accept_out, bu.block_len,
                          block_ind, force_accept=force_accept)

    # ---- internals
    def _block_len(self, n_blocks):
        nvar = self._model.prior.nvar
        if isinstance(n_blocks, int):
            block_len = nvar // n_blocks
            if n_blocks < 1 or block_len * n_blocks != nvar:
                raise AssertionError(f"n_blocks ({n_blocks}) must divide the number of sites ({nvar})")
            return block_len, n_blocks
        return nvar, 1

    @staticmethod
    def _check_field(x):
        if x.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"BlockedMCMCSampler supports float32 and float64 fields, got {x.dtype}")

    def _on_device(self, x):
        return x.is_cuda and not getattr(self._model.prior, 'torch_rng', True)

    def _start(self, n_chains):
        """Chains to continue (inverse flow of `_ref['sample']`) or fresh prior draws with logqp_ref None."""
        model, prior = self._model, self._model.prior
        s = self._ref['sample']
        want = tuple(prior.shape) if n_chains == 1 else (n_chains, *prior.shape)
        if s is not None and tuple(s.shape) == want:
            x = model.net_.backward(s.unsqueeze(0) if n_chains == 1 else s)[0]
            logqp_ref = self._ref['logqp']
        else:
            print("Starting from scratch & setting logqp_ref to None")
            x = prior.sample(n_chains)
            logqp_ref = None
        x = x.contiguous()
        self._check_field(x)
        return x, logqp_ref

    @staticmethod
    def _ref_tensor(logqp_ref, n, device):
        """logqp_ref as the (n) float64 device buffer nf_block_accept updates (a copy: `_ref` is left as it is)."""
        if logqp_ref is None:
            return torch.zeros(n, dtype=torch.float64, device=device)
        t = torch.as_tensor(logqp_ref, dtype=torch.float64).to(device).reshape(-1)
        return (t.expand(n) if t.numel() == 1 else t).clone()

    def _evaluate(self, x):
        model = self._model
        y, logJ = model.net_(x)
        return y, model.prior.log_prob(x) - logJ, -model.action(y)

    def _sweep_device(self, x, n_blocks, ref_t, flags, fresh):
        for k in range(n_blocks):
            self.step(x, k, ref_t, flags[k], force_accept=(fresh and k == 0))

    def _sweep_host(self, x, n_blocks, logqp_ref):
        """The reference's sweep (mcmc.py:199-220); with C > 1 chains every chain takes its own uniform and decision."""
        prior, net_, action = self._model.prior, self._model.net_, self._model.action
        n = x.shape[0]
        if n == 1:
            accept_seq = np.empty(n_blocks, dtype=bool)
            lrand_arr = np.log(np.random.rand(n_blocks))
        else:
            accept_seq = np.empty((n, n_blocks), dtype=bool)
            lrand_arr = np.log(np.random.rand(n_blocks, n))
            if logqp_ref is not None:
                logqp_ref = seize(torch.as_tensor(logqp_ref, dtype=torch.float64)).reshape(-1)
        for ind in range(n_blocks):
            prior.blockupdater(x, ind)  # in-place updater
            y, logJ = net_(x)
            logq = prior.log_prob(x) - logJ
            logp = -action(y)
            if n == 1:
                if ind == 0 and logqp_ref is None:
                    accept_seq[ind] = True
                else:
                    accept_seq[ind] = lrand_arr[ind] < logqp_ref - (logq - logp)[0]
                if accept_seq[ind]:
                    logqp_ref = (logq - logp).item()
                else:
                    prior.blockupdater.restore(x, ind)
                continue
            d = seize(logq - logp).astype(np.float64)
            ok = np.ones(n, dtype=bool) if (ind == 0 and logqp_ref is None) else lrand_arr[ind] < logqp_ref - d
            accept_seq[:, ind] = ok
            logqp_ref = d if logqp_ref is None else np.where(ok, d, logqp_ref)
            if not ok.all():
                prior.blockupdater.restore(x, ind, torch.as_tensor(~ok, device=x.device))
        if n > 1:
            logqp_ref = torch.as_tensor(logqp_ref, dtype=torch.float64)
        return accept_seq, logqp_ref
