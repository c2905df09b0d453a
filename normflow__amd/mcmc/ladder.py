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
from .hmc import HMCSampler, HMCHistory, _Span


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
    """`sample(batch_size, n_chains=C, n_md=10, dt=0.1, n_skip=0, exchange_every=1, path=None, integrator='leapfrog')`
    -> (batch_size, *L) (`integrator` as in HMCSampler, on sample, sample_ and measure alike),
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
    holds the chains' phi (C, *L), action (C) and rung (C) int32, indexed by chain.
    cluster_every = Ec (sample, sample_, measure; 0 = none, the sampler as it was): one Swendsen-Wang sweep of all chains,
    each under the hopping coefficient of the rung it holds, BEFORE every recorded step s with s % Ec == 0 (s counted
    across calls; `start` resets it).  The exchange sweep stays AFTER every E-th step and spans end at whichever boundary
    comes first; where both fall between the same two steps the exchange comes first and the cluster sweep uses the new
    rungs.  The path is `HMCSampler._sweep_path`'s: nf_phi4_cluster_ladder, nf_phi4_cluster_tiled_ladder (one workspace
    per call), or the composed `cluster_sweep` with coef[rung, 0] (its draws from nf_phi4_cluster_draws on the device,
    from torch's CPU generator on CPU tensors; on the composed HMC path S is recomputed under the chains' rungs after a
    sweep).  Philox positions in call order: 2 per trajectory, 1 per exchange, 2 per cluster sweep.  `last['cluster']`
    holds the sweeps' stats (sweeps, C, 4) int32 on the device, rung-ordered.  When measuring on the fused path the
    exchange still decides by the rows of the span's last launch: they are always taken after the last cluster sweep,
    because sweeps precede spans.  `cluster(phi, rung)` is the bare sweep."""

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
    def measure(self, batch_size=1, return_rows=False, improved=False, momenta=None, spectrum_path=None, modes=None,
                modes_path=None, **kwargs):
        """The list of K `Measurement`s.  improved=True / 'kernel' / 'composed' / 'hbm' as in `HMCSampler.measure`: entry k then
        carries `.improved`, the `ImprovedMeasurement` of rung k's sweeps x R rows (the kernel does not know the
        couplings: a sweep's C rows are taken by chain and laid out rung-ordered, row (c // K) K + rung[c] with the rungs
        in force at that sweep, like `last['cluster']`).  momenta='all' or an int >= 1 as in `HMCSampler.measure`: the
        spectrum rides along, rung-ordered like the rest.  spectrum_path='hbm' and modes=[(n0, ...), ...] as in
        `HMCSampler.measure`: `.modes` and `.mode_power` ride along in the same way; modes_path='hbm' takes them from
        nf_cluster_modes_tiled, as there."""
        ipath = self._improved_path(improved, kwargs.get('cluster_every', 0))
        if momenta is not None and ipath is False:
            raise ValueError("momenta asks for the spectrum of the improved estimators: it needs improved=True (or a path)")
        self._spectrum_path(spectrum_path, momenta, ipath)
        y, rung_stats = self._advance(batch_size, want_rows=return_rows, want_stats=True, improved=ipath, momenta=momenta,
                                      spectrum_path=spectrum_path, **self._modes_kw(modes, ipath, modes_path), **kwargs)
        stats = rung_stats.out
        from ..lib import observables as ob
        K = len(self._ladder)
        lat = tuple(self._ref['sample'].shape[1:])
        ms = []
        for k in range(K):
            rows = stats[:, k::K].flatten(0, 1)                    # (steps R, n_out): step-major, the samplers' layout
            ms.append(ob.Measurement(*ob._split(rows, lat), lat, self._ladder.rung(k)))
            if ipath is not False:
                im, C = rung_stats.improved, self._ref['sample'].shape[0]
                pick = lambda t: t.reshape((-1, C) + tuple(t.shape[1:]))[:, k::K].flatten(0, 1)    # (sweeps R, ...)
                ms[k].improved = im.pick(pick)
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

    @torch.no_grad()
    def cluster(self, phi, rung=None, position=None, path=None):
        """ONE Swendsen-Wang sweep of the chains phi (C, *L), C a multiple of K, chain c under the hopping coefficient of
        rung[c] ((C) integers; None: the identity state c % K); phi and the stored chains are left alone.  Returns
        dict(phi, labels, stats) as `HMCSampler.cluster`, phi and labels by chain and stats (C, 4) RUNG-ORDERED: the row of
        chain c is (c // K) K + rung[c].  `position` and `path` as in `HMCSampler.cluster`; 'kernel' and 'tiled' are
        nf_phi4_cluster_ladder and nf_phi4_cluster_tiled_ladder."""
        K, C = len(self._ladder), phi.shape[0]
        if C < K or C % K != 0:
            raise ValueError(f"cluster: the {C} chains are not a positive multiple of the K = {K} rungs")
        rung = torch.arange(C, device=phi.device) % K if rung is None else torch.as_tensor(rung, device=phi.device)
        if tuple(rung.shape) != (C,):
            raise ValueError(f"cluster: rung must be ({C},), one rung per chain, got {tuple(rung.shape)}")
        coef = self._ladder.coef_table(tuple(phi.shape[1:]), phi.device)
        new, stats, labels = self._sweep(phi.detach(), (coef, rung.to(torch.int32).contiguous()), position=position,
                                         want_labels=True, path=path)
        return dict(phi=new, labels=labels, stats=stats)

    def _sweep(self, phi, couplings, position=None, want_labels=False, path=None, workspace=None):
        """HMCSampler's with `couplings` = (coef, rung) and the stats rung-ordered on every path: the ladder kernels write
        them so, the composed sweep's are laid out by the column (c // K) K + rung[c] here."""
        coef, rung = couplings
        out = super()._sweep(phi, position=position, want_labels=want_labels, path=path, workspace=workspace,
                             couplings=couplings)
        if self._sweep_path(phi, path) != 'composed':
            return out
        K = coef.shape[0]
        col = (torch.arange(phi.shape[0], device=phi.device) // K) * K + rung.long().clamp(0, K - 1)
        return (out[0], torch.empty_like(out[1]).index_copy_(0, col, out[1])) + tuple(out[2:])

    def trajectory(self, *args, **kwargs):
        raise NotImplementedError("LadderHMCSampler has no single-trajectory entry: use _hip.phi4_hmc_ladder(scheme=...) "
                                  "or model.hmc.trajectory(integrator=...) with the rung's action")

    # ---- which path: HMCSampler's `_choose`, on the proxy model (whose action is a phi^4 action)
    def _advance(self, batch_size, n_chains=None, n_md=10, dt=0.1, n_skip=0, exchange_every=1, path=None, want_rows=True,
                 want_stats=False, cluster_every=0, improved=False, integrator='leapfrog', momenta=None,
                 spectrum_path=None, fa_mass_sq=None, modes=None, modes_path=None):
        """batch_size // C recorded steps.  Returns (the rung-ordered rows or None, the `_RungStats` with the rung-ordered
        measure rows `out` (steps, C, n_out) or None)."""
        if fa_mass_sq is not None:
            raise TypeError("model.hmc.ladder(...) does not take fa_mass_sq: a(k) = 1 / (w0 khat^2 + M^2) would depend on "
                            "the rung a chain holds; Fourier acceleration runs on model.hmc with one action")
        K = len(self._ladder)
        C = int(K if n_chains is None else n_chains)
        if C < 1 or C % K != 0:
            raise ValueError(f"n_chains ({C}) must be a positive multiple of the K = {K} rungs")
        C, n_md, every, E = self._checked(batch_size, C, n_md, n_skip, exchange_every, 'exchange_every')
        Ec = self._checked(batch_size, C, n_md, n_skip, cluster_every, 'cluster_every')[3]
        scheme = self._scheme(integrator)
        self._restart(C)
        phi, S, rung = self._ref['sample'].clone(), self._ref['action'], self._ref['rung'].clone()
        path = self._choose(phi, path)
        dev, lat = phi.device, tuple(phi.shape[1:])
        rows = batch_size // C
        coef = self._ladder.coef_table(lat, dev)
        base = (torch.arange(C, device=dev) // K) * K
        out = torch.empty((rows, C) + lat, dtype=phi.dtype, device=dev) if want_rows else None
        stats = _RungStats(rows, C, lat, dev) if want_stats else None
        ws = self._tiled_workspace(phi) if path == 'tiled' else None
        sweep_ws = None
        if Ec and self._sweep_path(phi) == 'tiled':      # one workspace for all sweeps of the call
            need = _hip.cluster_tiled_workspace(C, lat)
            sweep_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=dev)
        if improved is not False:
            from ..lib.observables import ImprovedMeasurement, measure_improved
            spec = self._spectrum_workspace(phi, momenta, spectrum_path)      # one workspace for all sweeps of the call
            if modes is not None:
                spec = dict(spec, modes=modes, **self._modes_workspace(phi, modes, modes_path))
                modes = _hip.modes_reduced(lat, modes)   # what an empty measurement carries
        dhs, accs, swaps, parities, sweeps, parts = [], [], [], [], [], []
        r0 = 0
        while r0 < rows:
            self._ref['rung'] = rung                     # what the composed path's action reads
            if Ec and self._steps % Ec == 0:             # after the exchange that fell between the same two steps
                if improved is False:
                    phi, st = self._sweep(phi, (coef, rung), workspace=sweep_ws)
                else:                                    # the same sweep, its labels kept; the rows rung-ordered
                    phi, st, labels = self._sweep(phi, (coef, rung), workspace=sweep_ws, want_labels=True)
                    parts.append(measure_improved(phi, labels, path=improved, momenta=momenta, **spec).rows(base + rung.long()))
                sweeps.append(st)
                if path == 'composed':
                    S = self._model.action(phi.double()).double()
            g = self._span(self._steps, self._span(self._steps, rows - r0, E), Ec)
            col = base + rung.long()                     # the rung-ordered column of every chain
            if stats is not None:
                stats.col = col
            sink = _Span(out, stats, r0, col)
            if path == 'composed':
                S = self._run_composed(phi, S, g, every, n_md, dt, sink, dhs, accs, col, scheme)
            else:
                S = self._run(path, phi, (coef, rung), g, every, n_md, dt, ws, sink, dhs, accs, scheme)
            r0 += g
            self._steps += g
            if E and self._steps % E == 0 and K > 1:
                # the chains' measure rows: the span's last where it measured, else the chains measured where they lie
                chain_rows = stats.chain_rows if stats is not None else measure_rows(phi)
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
        swapped = torch.stack(swaps) if swaps else torch.zeros((0, C // K, K - 1), dtype=torch.uint8, device=dev)
        accepted = self._finish(dhs, accs, extra=swapped.double().sum(dim=(0, 1)), scheme=scheme)    # the accepted swaps per pair
        self.last['swapped'] = swapped
        if Ec:
            self.last['cluster'] = (torch.stack(sweeps) if sweeps else
                                    torch.empty((0, C, 4), dtype=torch.int32, device=dev))
        if improved is not False:                 # only `measure` asks, so there are stats to carry the rows
            stats.improved = ImprovedMeasurement.cat(parts, lat, dev,
                                                     None if momenta is None else _hip.spectrum_momenta(lat, momenta), modes)
        tried = [sum(1 for p in parities if p == k % 2) * (C // K) for k in range(K - 1)]
        self.history.exchange_rate.append([n / t if t else float('nan') for n, t in zip(accepted, tried)])
        y = None if out is None else out.reshape((batch_size,) + lat)
        return y, stats

    def _run_composed(self, phi, S, rows, every, n_md, dt, sink, dhs, accs, col, scheme=None):
        """HMCSampler's, with the chains updated in place and dH and the accept flags rung-ordered.  Returns S."""
        for t in range(rows * every):
            phi_new, S, dh, acc, _ = self._trajectory_composed(phi, S, n_md, dt, scheme=scheme)
            phi.copy_(phi_new)
            dhs.append(torch.empty_like(dh).index_copy_(0, col, dh).unsqueeze(0))
            accs.append(torch.empty_like(acc).index_copy_(0, col, acc).unsqueeze(0))
            if (t + 1) % every == 0:
                sink.take((t + 1) // every - 1, phi)
        return S


class _RungStats:
    """`hmc._Stats` for the ladder: the rung-ordered measure rows `out` (steps, C, n_out) of a call.  `col` is the column
    of every chain during the span being written, `chain_rows` the chains' own rows (C, n_out) after the last step
    written: the exchange sweep decides by them."""

    def __init__(self, rows, C, lat, device):
        self.out = torch.empty((rows, C, _hip.measure_n_out(lat)), dtype=torch.float64, device=device)
        self.col = self.chain_rows = None
        self.improved = None            # the call's rung-ordered ImprovedMeasurement, where `measure(improved=...)` asked

    def put(self, r, phi):
        """Step r: the chains as they lie."""
        self.chain_rows = measure_rows(phi)
        self.out[r].index_copy_(0, self.col, self.chain_rows)

    def put_rows(self, r0, block):
        """Steps r0 ..: (k, C, n_out) rows measured inside a launch, rung-ordered as they come."""
        self.out[r0:r0 + block.shape[0]] = block
        self.chain_rows = block[-1][self.col]             # rung-ordered -> by chain
