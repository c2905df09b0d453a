"""Hybrid Monte Carlo along a coupling ladder, with replica exchange (MI355X-side extension, no counterpart in the
reference): `model.hmc.ladder(ScalarPhi4Ladder(...))`.

C = K R chains: chain c belongs to replica set c // K and holds rung rung[c] of the ladder's K couplings; within a set the
rungs are a permutation of 0 .. K - 1 (`start` sets rung[c] = c % K).  Every chain runs the HMC of mcmc/hmc.py under the
couplings of its rung -- one launch for all of them, the coefficients looked up per chain (nf_phi4_hmc_ladder,
nf_phi4_hmc_tiled_ladder) -- and an exchange sweep (nf_phi4_ladder_exchange) lets the two chains on neighbouring rungs
trade their RUNGS with the Metropolis probability min(1, exp(Delta)),
    Delta = (w2_k - w2_{k+1}) (Q_a - Q_b) + (w4_k - w4_{k+1}) (P_a - P_b) - (w0_k - w0_{k+1}) (Lam_a - Lam_b),
Q = sum phi^2, P = sum phi^4, Lam = the sum of the links of the chain a on rung k and the chain b on rung k + 1: the action
is linear in the couplings, so the decision needs the chains' measure rows and nothing else, and no configuration moves.
Everything a caller sees is RUNG-ORDERED: column set K + k of a step is the chain of that set that holds rung k then."""
import torch

from .. import _hip
from ..action.scalar_action import ScalarPhi4Action
from .hmc import HMCSampler, HMCHistory


def exchange_sweep(rows, coef, rung, action, parity, logu):
    """One exchange sweep from torch ops, the rule of nf_phi4_ladder_exchange (include/normflow_hip.h) on any device: rows
    (C, >= 7) float64 are the chains' measure rows, coef (K, 3) float64, rung (C) integer, action (C) float64 or None, logu
    (C // K, K - 1) float64 with entry (set, k) the log of the uniform of the pair (k, k + 1).  Returns (the new rung, the
    new action or None, swapped (C // K, K - 1) uint8); nothing is changed in place.  The composed path on CPU tensors
    decides by this."""
    K = coef.shape[0]
    R = rung.shape[0] // K
    swapped = torch.zeros((R, max(K - 1, 0)), dtype=torch.uint8, device=rung.device)
    ks = torch.arange(int(parity), max(K - 1, int(parity)), 2, device=rung.device)
    if ks.numel() == 0:
        return rung.clone(), None if action is None else action.clone(), swapped
    inv = torch.argsort(rung.reshape(R, K).long(), dim=1)                      # inv[set, k]: the chain (in its set) on rung k
    base = (torch.arange(R, device=rung.device) * K).unsqueeze(1)
    a, b = base + inv[:, ks], base + inv[:, ks + 1]                            # (R, pairs) chain indices
    sums = torch.stack([rows[:, 3:7].sum(dim=1), rows[:, 1], rows[:, 2]], dim=1)   # (C, 3): Lam, Q, P
    sign = torch.tensor([-1.0, 1.0, 1.0], dtype=torch.float64, device=rows.device)
    dw = (coef[ks] - coef[ks + 1]) * sign                                      # (pairs, 3)
    delta = ((sums[a] - sums[b]) * dw.unsqueeze(0)).sum(dim=2)                 # (R, pairs)
    ok = logu[:, ks] < delta
    swapped[:, ks] = ok.to(torch.uint8)
    new_rung = rung.clone()
    rk = ks.to(rung.dtype).unsqueeze(0).expand_as(a)
    new_rung[a] = torch.where(ok, rk + 1, rk)
    new_rung[b] = torch.where(ok, rk, rk + 1)
    new_action = None
    if action is not None:
        new_action = action.clone()
        S = lambda c, k: (sums[c] * (coef[k] * sign)).sum(dim=2)               # w2 Q + w4 P - w0 Lam of the chains c on rungs k
        ka, kb = (ks + 1).unsqueeze(0).expand_as(a), ks.unsqueeze(0).expand_as(b)
        new_action[a] = torch.where(ok, S(a, ka), action[a])
        new_action[b] = torch.where(ok, S(b, kb), action[b])
    return new_rung, new_action, swapped


def measure_rows(phi):
    """The (C, 7 + sum of the four padded extents) float64 rows of the chains phi (C, *L) in nf_lattice_measure's layout,
    by the path that `observables.route` names: either kernel, else the composed sums laid out the same way."""
    from ..lib import observables as ob
    path = ob.route(phi)
    if path == 'kernel':
        return _hip.lattice_measure(phi.contiguous())
    if path == 'tiled':
        return _hip.lattice_measure_tiled(phi.contiguous())
    scalars, links, slices = ob._compose(phi)
    pad = 4 - (phi.ndim - 1)
    zeros = torch.zeros((phi.shape[0], pad), dtype=torch.float64, device=phi.device)
    own = scalars[:, :1].expand(-1, pad)                    # the one slice of a padding axis of extent 1 is sum phi
    return torch.cat([scalars, zeros, links, own] + list(slices), dim=1)


class LadderHistory(HMCHistory):
    _KEYS = HMCHistory._KEYS + ('exchange_rate',)


class _RungAction(ScalarPhi4Action):
    """The ladder's action at the rungs the sampler's chains hold now: what HMCSampler's composed path and its `start`
    call as `model.action` (a phi^4 action whose couplings differ per row)."""

    def __init__(self, sampler):
        self._sampler = sampler

    def action(self, cfgs):
        s = self._sampler
        return s._ladder.action(cfgs, s._ref['rung'])

    __call__ = action


class _LadderModel:
    def __init__(self, model, sampler):
        self.prior = model.prior
        self.action = _RungAction(sampler)


class LadderHMCSampler(HMCSampler):
    """`sample(batch_size, n_chains=C, n_md=10, dt=0.1, n_skip=0, exchange_every=1, path=None)` -> (batch_size, *L),
    RUNG-ORDERED: row r is recorded step r // C, column r % C = set K + rung.  C must be a multiple of K = len(ladder)
    and batch_size of C.  `split(y)` -> (K, batch_size / K, *L): entry k is rung k's rows in the samplers' layout for
    n_chains = R = C / K.  `measure(...)` takes the same arguments and returns a list of K `Measurement`s, entry k that of
    rung k with the action of `ladder.rung(k)`; `Ensemble(ms[k], n_chains=R)` takes it as is; nothing is stored.
    exchange_every = E: after every E-th recorded step (counted across calls; `start` resets the count) one exchange
    sweep, of alternating parity; E = 0: none.  Between two sweeps the trajectories are one ladder launch, or as few as
    the work caps allow.  The rows a sweep decides by are the chains' measure rows: when measuring on the fused path the
    last rows measured inside the launch, which are rung-ordered and are indexed back to the chains by `rung` on the
    device; otherwise the chains are measured where they lie, by the path `observables.route` names.
    Paths as in HMCSampler: fused and tiled run the ladder kernels; composed runs the same algorithm with
    `ladder.action` and per-row coefficients (on CPU tensors the exchange uniforms come from torch's CPU generator, K - 1
    per replica set and sweep).  On the device all three use the same Philox positions of torch's CUDA generator, in call
    order: 2 per trajectory and 1 per sweep.  Nothing is read back from the device inside the loop; the one read per call
    fills `history` (accept_rate, exp_mdh, dh_rms and exchange_rate: K - 1 rates accepted / tried, nan where a pair was
    never tried).  `last` holds dh and accept (trajectories, C), rung-ordered, and swapped (sweeps, R, K - 1); `_ref`
    holds the chains' phi (C, *L), action (C) and rung (C) int32, indexed by chain."""

    def __init__(self, model, ladder):
        if len(ladder) < 1:
            raise ValueError("LadderHMCSampler needs a ladder of at least one rung")
        self._ladder = ladder
        super().__init__(_LadderModel(model, self))
        self.history = LadderHistory()
        self._ref = dict(sample=None, action=None, rung=None)
        self.last = dict(dh=None, accept=None, swapped=None)
        self._steps = self._sweeps = 0

    def __len__(self):
        return len(self._ladder)

    # ---- public
    @torch.no_grad()
    def sample(self, batch_size=1, **kwargs):
        return self._advance(batch_size, want_rows=True, want_stats=False, **kwargs)[0]

    @torch.no_grad()
    def sample_(self, batch_size=1, **kwargs):
        """(y, logp): logp = -S(y) under the rung of every row, in the field dtype."""
        y = self.sample(batch_size, **kwargs)
        K = len(self._ladder)
        rung = torch.arange(y.shape[0], device=y.device) % K
        return y, (-self._ladder.action(y, rung)).to(y.dtype)

    @torch.no_grad()
    def measure(self, batch_size=1, return_rows=False, **kwargs):
        y, stats = self._advance(batch_size, want_rows=return_rows, want_stats=True, **kwargs)
        from ..lib import observables as ob
        K = len(self._ladder)
        lat = tuple(self._ref['sample'].shape[1:])
        ms = []
        for k in range(K):
            rows = stats[:, k::K].flatten(0, 1)                    # (steps R, n_out): step-major, the samplers' layout
            ms.append(ob.Measurement(*ob._split(rows, lat), lat, self._ladder.rung(k)))
        return (ms, y) if return_rows else ms

    def split(self, y):
        """Rung-ordered rows (batch_size, *L) -> (K, batch_size / K, *L), entry k in the samplers' layout for R chains."""
        K = len(self._ladder)
        if y.shape[0] % K != 0:
            raise ValueError(f"split: {y.shape[0]} rows are not a multiple of the K = {K} rungs")
        return y.reshape((y.shape[0] // K, K) + tuple(y.shape[1:])).transpose(0, 1).contiguous()

    @torch.no_grad()
    def start(self, phi=None, n_chains=None):
        """Start the chains from phi (C, *L) or from model.prior.sample(n_chains), on the identity ladder state
        rung[c] = c % K; the counts of recorded steps and of sweeps (the sweeps' parity) start again."""
        K = len(self._ladder)
        C = int(phi.shape[0] if phi is not None else K if n_chains is None else n_chains)
        if C < K or C % K != 0:
            raise ValueError(f"n_chains ({C}) must be a positive multiple of the K = {K} rungs")
        if phi is None:
            phi = self._model.prior.sample(C)
        self._ref['rung'] = (torch.arange(C, device=phi.device) % K).to(torch.int32)
        self._steps = self._sweeps = 0
        return super().start(phi)

    def trajectory(self, *args, **kwargs):
        raise NotImplementedError("LadderHMCSampler has no single-trajectory entry: use _hip.phi4_hmc_ladder or "
                                  "model.hmc.trajectory with the rung's action")

    # ---- which path: HMCSampler's `_choose`, on the proxy model (whose action is a phi^4 action)
    def _advance(self, batch_size, n_chains=None, n_md=10, dt=0.1, n_skip=0, exchange_every=1, path=None, want_rows=True,
                 want_stats=False):
        """batch_size // C recorded steps.  Returns (the rung-ordered rows or None, the rung-ordered measure rows
        (steps, C, n_out) or None)."""
        K = len(self._ladder)
        C = int(K if n_chains is None else n_chains)
        if C < 1 or C % K != 0:
            raise ValueError(f"n_chains ({C}) must be a positive multiple of the K = {K} rungs")
        if batch_size < 1 or batch_size % C != 0:
            raise ValueError(f"batch_size ({batch_size}) must be a positive multiple of n_chains ({C})")
        n_md, every, E = int(n_md), int(n_skip) + 1, int(exchange_every)
        if n_md < 1 or every < 1 or E < 0:
            raise ValueError(f"n_md ({n_md}) must be >= 1, n_skip ({n_skip}) >= 0 and exchange_every ({exchange_every}) >= 0")
        s = self._ref['sample']
        if s is None or s.shape[0] != C:
            print("Starting from scratch")
            self.start(n_chains=C)
        phi, S, rung = self._ref['sample'].clone(), self._ref['action'], self._ref['rung'].clone()
        path = self._choose(phi, path)
        dev, lat = phi.device, tuple(phi.shape[1:])
        rows = batch_size // C
        coef = self._ladder.coef_table(lat, dev)
        base = (torch.arange(C, device=dev) // K) * K
        out = torch.empty((rows, C) + lat, dtype=phi.dtype, device=dev) if want_rows else None
        n_out = 7 + sum(lat) + 4 - len(lat)
        stats = torch.empty((rows, C, n_out), dtype=torch.float64, device=dev) if want_stats else None
        ws = None
        if path == 'tiled':
            need = _hip.load().nf_phi4_hmc_tiled_workspace(C, _hip._lat4(lat), _hip._dtype_code(phi))
            ws = torch.empty(max(int(need), 256), dtype=torch.uint8, device=dev)
        dhs, accs, swaps, parities = [], [], [], []
        r0 = 0
        while r0 < rows:
            g = rows - r0 if E == 0 else min(rows - r0, E - self._steps % E)
            self._ref['rung'] = rung                     # what the composed path's action reads
            S, chain_rows = self._block(path, phi, S, coef, rung, base, g, every, n_md, dt, ws,
                                        None if out is None else out[r0:r0 + g], None if stats is None else stats[r0:r0 + g],
                                        dhs, accs)
            r0 += g
            self._steps += g
            if E and self._steps % E == 0 and K > 1:
                if chain_rows is None:
                    chain_rows = measure_rows(phi)
                parity = self._sweeps % 2
                if phi.is_cuda:
                    S = S.contiguous()
                    swaps.append(_hip.ladder_exchange(chain_rows, coef, rung, parity, action=S))
                else:
                    logu = torch.log(1.0 - torch.rand((C // K, K - 1), dtype=torch.float64, device=dev))    # u in (0, 1]
                    rung, S, sw = exchange_sweep(chain_rows, coef, rung, S, parity, logu)
                    swaps.append(sw)
                parities.append(parity)
                self._sweeps += 1
        self._ref.update(sample=phi, action=S, rung=rung)
        dh, acc = torch.cat(dhs), torch.cat(accs)
        swapped = torch.stack(swaps) if swaps else torch.zeros((0, C // K, K - 1), dtype=torch.uint8, device=dev)
        self.last = dict(dh=dh, accept=acc, swapped=swapped)
        # the one read: the three HMC statistics and the accepted swaps per pair
        got = torch.cat([torch.stack([acc.double().mean(), torch.exp(-dh).mean(), dh.square().mean().sqrt()]),
                         swapped.double().sum(dim=(0, 1))]).cpu().tolist()
        for key, val in zip(HMCHistory._KEYS, got[:3]):
            getattr(self.history, key).append(val)
        tried = [sum(1 for p in parities if p == k % 2) * (C // K) for k in range(K - 1)]
        self.history.exchange_rate.append([n / t if t else float('nan') for n, t in zip(got[3:], tried)])
        y = None if out is None else out.reshape((batch_size,) + lat)
        return y, stats

    def _block(self, path, phi, S, coef, rung, base, g, every, n_md, dt, ws, out, stats, dhs, accs):
        """g recorded steps of the chains phi (in place) under the rungs `rung`, in as few launches as the caps allow; the
        rung-ordered rows go to out (g, C, *L) and stats (g, C, n_out) where given, dh and accept to the lists.  Returns
        (S (C) of the chains, the chains' measure rows after the last step where they are at hand, else None)."""
        C, V = phi.shape[0], phi[0].numel()
        col = (base + rung.long())                        # the rung-ordered column of every chain
        chain_rows = None

        def put(dst, r, values):                          # chain-indexed values into the rung-ordered row r
            dst[r].index_copy_(0, col, values)

        if path == 'composed':
            for t in range(g * every):
                phi_new, S, dh, acc, _ = self._trajectory_composed(phi, S, n_md, dt)
                phi.copy_(phi_new)
                dhs.append(torch.empty_like(dh).index_copy_(0, col, dh).unsqueeze(0))
                accs.append(torch.empty_like(acc).index_copy_(0, col, acc).unsqueeze(0))
                if (t + 1) % every == 0:
                    r = (t + 1) // every - 1
                    if out is not None:
                        put(out, r, phi)
                    if stats is not None:
                        chain_rows = measure_rows(phi)
                        put(stats, r, chain_rows)
            return S, chain_rows
        fused = path == 'fused'
        if fused:
            steps = _hip.HMC_MAX_WORK // (max(V, 256) * ((C + 1023) // 1024))            # the MD steps of one launch
            group = every * n_md + (_hip.HMC_MEASURE_MD_STEPS if stats is not None else 0)
            fit = steps // group
            per = max(1, steps // n_md)
        else:
            per = max(1, _hip.HMC_TILED_MAX_LAUNCHES // (n_md + 2))
            fit = per // every if stats is None else min(1, per // every)     # measured where they lie: a call per step
        kw = dict(workspace=ws) if not fused else {}
        kernel = _hip.phi4_hmc_ladder if fused else _hip.phi4_hmc_tiled_ladder
        r = None
        if fit >= 1:
            r0 = 0
            while r0 < g:
                k = min(fit, g - r0)
                if fused:
                    kw = dict(measure=stats is not None, record=out is not None)
                elif out is None:
                    kw = dict(workspace=ws)
                r = kernel(phi, coef, rung, n_md, dt, n_traj=k * every,
                           record_every=every if (fused or out is not None) else None, **kw)
                dhs.append(r['dh']); accs.append(r['accept'])
                if out is not None:
                    out[r0:r0 + k] = r['record']
                if stats is not None:
                    if fused:
                        stats[r0:r0 + k] = r['measure']
                        chain_rows = r['measure'][-1][col]          # rung-ordered -> by chain
                    else:
                        chain_rows = measure_rows(phi)
                        put(stats, r0, chain_rows)
                r0 += k
        else:
            # one recorded step is more than a launch: unrecorded launches, the step taken from the chains where they lie
            for r0 in range(g):
                left = every
                while left:
                    k = min(per, left)
                    r = kernel(phi, coef, rung, n_md, dt, n_traj=k, **({} if fused else dict(workspace=ws)))
                    dhs.append(r['dh']); accs.append(r['accept'])
                    left -= k
                if out is not None:
                    put(out, r0, phi)
                if stats is not None:
                    chain_rows = measure_rows(phi)
                    put(stats, r0, chain_rows)
        return r['action'], chain_rows
