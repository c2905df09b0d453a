"""Hybrid Monte Carlo on the target exp(-S) itself (MI355X-side extension, no counterpart in the reference): an exact
sampler that does not go through the flow, for checking what the flow-based samplers produce at lambda != 0, for seeding
them and for making training configurations.

One definition, three implementations.  For C independent chains, per trajectory:
    F(phi) = dS/dphi;  pi ~ N(0, 1);  H0 = sum pi^2 / 2 + S(phi)
    pi -= (dt / 2) F(phi);  k = 1 .. n_md: phi += dt pi, pi -= (dt, or dt / 2 when k = n_md) F(phi)
    H1 likewise;  accept iff log u < -(H1 - H0), u in (0, 1];  a rejected chain keeps its phi bit for bit.
The energies are taken in double whatever the field dtype.
That is leapfrog, the default `integrator`.  In general an integrator is a scheme of s stages of drift weights a and kick
weights b (include/normflow_hip.h, "integration schemes"; `_hip.hmc_scheme`): 'leapfrog', 'omelyan' (second-order
minimum norm, s = 2), 'omf4' (fourth order, s = 5) or a pair (a, b), and a trajectory is
    pi -= (b_s / 2) dt F(phi);  k = 1 .. n_md, j = 1 .. s: phi += a_j dt pi, pi -= b_j dt F(phi)
    (b_s / 2 instead of b_s at the very end)
with n_md s force evaluations, the same two random draws and no more memory, on all three implementations.
  * fused:    nf_phi4_hmc (nf_hmc.hip), a whole run of trajectories of a chain in one launch with the chain resident in a
              CU -- ScalarPhi4Action on a HIP device, lattices nf_phi4_hmc_supported takes;
  * tiled:    nf_phi4_hmc_tiled (nf_hmc_tiled.hip), the chains in HBM and many workgroups per chain, n_md + 2 launches per
              trajectory (begin, n_md fused leapfrog steps, commit) -- ScalarPhi4Action on a HIP device, any lattice of
              one to four axes: the lattices beyond the fused kernel's 64 KiB image (32^3, 16^4, 32^4, 48^4);
  * composed: the same algorithm from the pieces the package already has (nf_normal_sample for the momenta, the force by
              autograd through `model.action`, torch ops for the updates, nf_block_accept for the decision and the
              restore) -- any lattice, any action object; on CPU tensors with torch's CPU generator.
On the device all three draw from the same Philox positions of torch's CUDA generator (two per trajectory: momenta,
uniform), so from the same seed they walk the same chain up to rounding.

Fourier acceleration (`fa_mass_sq=M2` on sample, sample_, measure and trajectory; None = everything above, call for call):
the kinetic term becomes pi^T A pi / 2 with A = T diag(a) T diagonal in momentum space, a(k) = 1 / (w0 khat^2 + M2), so
that every mode of the quadratic part of the action turns at nearly the same rate (include/normflow_hip.h,
"Fourier-accelerated hybrid Monte Carlo"):
    pi = A^(-1/2) eta, eta ~ N(0, 1);  H = sum pi (A pi) / 2 + S(phi);  phi += a_j dt (A pi);  pi -= b_j dt F(phi)
  * fa:       nf_phi4_hmc_fa (nf_hmc_fa.hip), the chain and the Hartley transform resident in a CU -- ScalarPhi4Action on
              a HIP device, lattices nf_phi4_hmc_fa_supported takes;
  * composed: the same rule from torch ops, the filter through torch.fft.rfftn / irfftn with a(k) from the shared table
              (`_hip.hmc_fa_table`) -- everywhere else: CPU tensors, lattices beyond one CU, any action with a `get_coef`;
  * fa_tiled: nf_phi4_hmc_fa_tiled (nf_hmc_fa_tiled.hip), the chains in HBM, the filter in 2 g - 1 passes over panels of
              g groups of axes and the tiled step with the velocity as an operand -- ScalarPhi4Action on a HIP device,
              lattices nf_phi4_hmc_fa_tiled_supported takes (every extent <= 64: 32^3, 16^4, 32^4, 48^4, 64^3).  OPT-IN:
              only `path='fa_tiled'` runs it; path=None chooses between 'fa' and 'composed' as it always did.
Cluster sweeps fall between launches and do not see the kinetic term."""
import torch

from .. import _hip
from ..action.scalar_action import ScalarPhi4Action
from .schedule import Take, schedule, schedule_fa


class HMCHistory:
    _KEYS = ('accept_rate', 'exp_mdh', 'dh_rms')

    def __init__(self):
        self.reset_history()

    def reset_history(self):
        for k in self._KEYS:
            setattr(self, k, [])


class HMCSampler:
    """`sample(batch_size, n_chains=C, n_md=10, dt=0.1, n_skip=0, path=None, integrator='leapfrog')` -> (batch_size, *L): row r is recorded
    trajectory r // C of chain r % C (the layout of the other samplers), with n_skip unrecorded trajectories before every
    recorded one.  `_ref` keeps the chains' phi (C, *L) and S (C) float64; the next call continues them, `start()` sets
    them.  `path`: None = the fused kernel where it applies, else the tiled kernels where they apply (they beat the composed path on
    every shape class measured, README), else composed; 'fused' / 'tiled' / 'composed' force one.
    `history` gets, per call, accept_rate, exp_mdh (the mean of exp(-dH), 1 for an exact integrator of the measure) and
    dh_rms, from one device-to-host read; `last` holds the call's dH and accept flags (trajectories, C) on the device.
    `measure(batch_size, ...)` walks the same chain and returns the `Measurement` of those rows without storing them: a
    run's length is then bounded by its 7 + sum L statistics per row, not by the rows.
    `cluster_every=E` (sample, sample_, measure; 0 = none, the sampler as it was): one Swendsen-Wang sweep of the signs of
    all chains (include/normflow_hip.h, "cluster updates") BEFORE the trajectories of every recorded step s with
    s % E == 0, s counted across calls since `start()`.  The launches are cut at the sweeps (at most E recorded steps
    each); the Philox positions are taken in call order, 2 per sweep and 2 per trajectory; a call still ends with an HMC
    launch, so `_ref`, `history` and `last['dh' | 'accept']` are the HMC's own, and `last['cluster']` holds the sweeps'
    stats (sweeps, C, 4) int32 on the device: clusters, sites flipped, largest cluster, and a positive count of the path
    that swept (-1: a loop bound was hit and the chain was left alone) -- the labelling rounds of nf_phi4_cluster and of
    the composed sweep, the tiles of a chain of nf_phi4_cluster_tiled.  The path is nf_phi4_cluster where
    `_hip.cluster_supported` takes the chains, nf_phi4_cluster_tiled on the classes of `cluster.TILED_CLASSES`, else the
    composed `cluster_sweep` (mcmc/cluster.py).  `cluster(phi)` is the bare sweep on given chains."""

    def __init__(self, model):
        self._model = model
        self.history = HMCHistory()
        self._ref = dict(sample=None, action=None)
        self.last = dict(dh=None, accept=None)
        self._steps = 0           # the recorded steps since `start()`: where the cluster sweeps fall

    # ---- public
    @torch.no_grad()
    def sample(self, batch_size=1, **kwargs):
        return self.sample_(batch_size=batch_size, **kwargs)[0]

    @torch.no_grad()
    def sample_(self, batch_size=1, n_chains=1, n_md=10, dt=0.1, n_skip=0, path=None, cluster_every=0,
                integrator='leapfrog', fa_mass_sq=None):
        """(y, logp): batch_size // n_chains recorded trajectories of every chain and logp = -S(y) in the field dtype.
        `integrator`: 'leapfrog', 'omelyan', 'omf4', a pair (a, b) of weights or an `_hip.HmcScheme`; anything but
        leapfrog is recorded in `last['integrator']` (the name, or the pair of weight tuples).
        `fa_mass_sq`: None, or M^2 > 0 of the Fourier-accelerated kinetic term (module docstring), recorded in
        `last['fa_mass_sq']`; `path` is then None, 'fa', 'composed' or (opt-in) 'fa_tiled'."""
        y, _ = self._advance(batch_size, n_chains, n_md, dt, n_skip, path, want_rows=True, want_stats=False,
                             cluster_every=cluster_every, integrator=integrator, **self._fa_kw(fa_mass_sq))
        return y, (-self._model.action(y)).to(y.dtype)

    @torch.no_grad()
    def measure(self, batch_size=1, n_chains=1, n_md=10, dt=0.1, n_skip=0, path=None, return_rows=False, cluster_every=0,
                improved=False, integrator='leapfrog', momenta=None, spectrum_path=None, fa_mass_sq=None, modes=None,
                modes_path=None):
        """The `Measurement` of the rows that `sample(batch_size, ...)` would return from the same chain and generator
        state, WITHOUT storing them: every recorded state is measured where it is and only its 7 + sum L sums are kept.
        The rows are in the samplers' layout (`Ensemble(m, n_chains=C)` takes it as is), the action is attached when the
        model's action is a ScalarPhi4Action (as `model.measure` does), and `_ref`, `history`, `last` and the generator
        are left as `sample_` leaves them.  On the device the tensors are those of `model.measure(hmc.sample(...))` bit
        for bit.  Per path:
          fused     nf_phi4_hmc_measure: the sums are taken from the kernel's LDS image inside the launch;
          tiled     per recorded step nf_phi4_hmc_tiled on the chains in place, then the measure kernel that
                    `observables.route` names for them, writing into that step's rows;
          composed  the same with the composed trajectory.
        return_rows=True: (Measurement, y), y as `sample` returns it.
        improved=True (or 'kernel' / 'composed' / 'hbm' to force a path of `observables.measure_improved`; 'hbm' is
        nf_cluster_moments_tiled, for the lattices beyond one CU's LDS, and opt-in): every cluster sweep
        of the call asks for its labels and the cluster-improved row of all chains is taken right after it; the
        Measurement then carries `.improved`, an `ImprovedMeasurement` of sweeps x C rows, row s C + c = sweep s of chain
        c (`ImprovedEnsemble(m.improved, n_chains=C)` takes it as is).  It needs cluster_every >= 1 (ValueError) and
        changes nothing else: the Measurement, the chains, `last`, `history` and the generator are those of the call
        without it bit for bit, and there is still one device-to-host read (the statuses stay on the device).
        momenta='all' or an int >= 1 (with improved; ValueError without): `.improved` also carries the cluster spectrum
        (`observables.measure_improved(..., momenta=...)`), from which the improved propagator and time-slice correlator
        follow; it changes nothing else of the call, bit for bit, `improved.out` included.
        spectrum_path='hbm' (with momenta; ValueError without; improved True or 'hbm'): the spectrum is
        nf_cluster_spectrum_tiled's (`observables.measure_improved(..., spectrum_path='hbm')`), for the lattices beyond
        one CU's LDS, with one workspace for all sweeps of the call.
        modes=[(n0, ...), ...] (with improved; ValueError without): `.improved` also carries `.modes` and `.mode_power`, the
        improved |phi~(p)|^2 at the listed momentum vectors, on or off the axes (`observables.measure_improved(...,
        modes=...)`, nf_cluster_modes); it changes nothing else of the call, bit for bit.
        modes_path='hbm' (with modes; ValueError without; improved True or 'hbm'): `.modes` and `.mode_power` are
        nf_cluster_modes_tiled's (`observables.measure_improved(..., modes_path='hbm')`), for the lattices beyond one CU's
        LDS, with one workspace for all sweeps of the call and no further device-to-host read.
        fa_mass_sq (as in `sample_`): the accelerated kernel does not measure inside its launch; its launches record
        the rows and they are measured afterwards by the kernel `observables.route` names, the same bits."""
        ipath = self._improved_path(improved, cluster_every)
        if momenta is not None and ipath is False:
            raise ValueError("momenta asks for the spectrum of the improved estimators: it needs improved=True (or a path)")
        self._spectrum_path(spectrum_path, momenta, ipath)
        y, stats = self._advance(batch_size, n_chains, n_md, dt, n_skip, path, want_rows=return_rows, want_stats=True,
                                 cluster_every=cluster_every, improved=ipath, integrator=integrator, momenta=momenta,
                                 spectrum_path=spectrum_path, **self._fa_kw(fa_mass_sq),
                                 **self._modes_kw(modes, ipath, modes_path))
        action = self._model.action
        m = stats.measurement(action if hasattr(action, 'get_coef') else None)
        if ipath is not False:
            m.improved = stats.improved
        return (m, y) if return_rows else m

    @staticmethod
    def _improved_path(improved, cluster_every):
        """False (no improved rows), or the `path` of `observables.measure_improved`: None, 'kernel', 'composed' or 'hbm'."""
        if improved is False or improved is None:
            return False
        if improved is not True and improved not in ('kernel', 'composed', 'hbm'):
            raise ValueError(f"improved must be False, True, 'kernel', 'composed' or 'hbm', got {improved!r}")
        if int(cluster_every) < 1:
            raise ValueError("improved estimators are taken from the labels of the cluster sweeps: improved needs "
                             f"cluster_every >= 1, got {cluster_every}")
        return None if improved is True else improved

    @staticmethod
    def _spectrum_path(spectrum_path, momenta, ipath):
        """The checks of `measure(spectrum_path=...)`, before anything runs: those of `observables.measure_improved`."""
        if spectrum_path is None:
            return
        if spectrum_path != 'hbm':
            raise ValueError(f"spectrum_path must be None or 'hbm', got {spectrum_path!r}")
        if momenta is None:
            raise ValueError("spectrum_path='hbm' is the path of the spectrum of the improved estimators: it needs momenta")
        if ipath not in (None, 'hbm'):
            raise ValueError(f"spectrum_path='hbm' goes with improved=True or 'hbm', got improved={ipath!r}")

    @staticmethod
    def _modes_kw(modes, ipath, modes_path=None):
        """The checks of `measure(modes=..., modes_path=...)`, before anything runs, and the keywords that hand them on;
        none at all for None, so that the calls are the ones they always were."""
        if modes_path is not None:
            if modes_path != 'hbm':
                raise ValueError(f"modes_path must be None or 'hbm', got {modes_path!r}")
            if modes is None:
                raise ValueError("modes_path='hbm' is the path of the modes of the improved estimators: it needs modes")
            if ipath not in (None, 'hbm'):
                raise ValueError(f"modes_path='hbm' goes with improved=True or 'hbm', got improved={ipath!r}")
        if modes is None:
            return {}
        if ipath is False:
            raise ValueError("modes asks for the improved estimators at a list of momenta: it needs improved=True (or a path)")
        if ipath == 'hbm' and modes_path is None:
            raise ValueError("modes: improved='hbm' has no HBM form of the modes of its own; modes_path='hbm' is "
                             "nf_cluster_modes_tiled, and improved=True or 'composed' take lattices beyond one CU on the "
                             "composed path")
        try:                                     # a tuple of tuples: `_hip.cluster_modes` then knows the list by one look-up
            modes = tuple(tuple(m) for m in modes)
        except TypeError:
            pass                                 # not a list of vectors: `measure_improved` says so
        return dict(modes=modes) if modes_path is None else dict(modes=modes, modes_path=modes_path)

    @staticmethod
    def _modes_workspace(phi, modes, modes_path):
        """One workspace of nf_cluster_modes_tiled for all sweeps of a call, and the keywords that hand it on."""
        if modes_path is None:
            return {}
        if not phi.is_cuda:
            raise _hip.NormflowHipError("modes_path='hbm' is nf_cluster_modes_tiled: it needs chains on the device")
        Cn, lat = phi.shape[0], tuple(phi.shape[1:])
        try:
            need = _hip.cluster_modes_tiled_workspace(Cn, lat, modes, 0, _hip.cluster_modes_tiled_per_pass(Cn, lat, modes))
        except _hip.NormflowHipError as e:
            raise ValueError(f"modes: {e}") from None
        return dict(modes_path=modes_path,
                    modes_workspace=torch.empty(max(need, 256), dtype=torch.uint8, device=phi.device))

    @staticmethod
    def _spectrum_workspace(phi, momenta, spectrum_path):
        """One workspace of nf_cluster_spectrum_tiled for all sweeps of a call, and the keywords that hand it on."""
        if spectrum_path is None:
            return {}
        if not phi.is_cuda:
            raise _hip.NormflowHipError("spectrum_path='hbm' is nf_cluster_spectrum_tiled: it needs chains on the device")
        Cn, lat = phi.shape[0], tuple(phi.shape[1:])
        need = _hip.cluster_spectrum_tiled_workspace(Cn, lat, momenta, 0, _hip.cluster_spectrum_tiled_per_pass(Cn, lat, momenta))
        return dict(spectrum_path=spectrum_path, workspace=torch.empty(max(need, 256), dtype=torch.uint8, device=phi.device))

    @staticmethod
    def _fa_kw(fa_mass_sq):
        """The keyword that hands fa_mass_sq on; none at all for None, so that the calls are the ones they always were."""
        return {} if fa_mass_sq is None else dict(fa_mass_sq=fa_mass_sq)

    @staticmethod
    def _scheme(integrator):
        """None for leapfrog by its name (the samplers then make the calls they always made), else the `_hip.HmcScheme`."""
        return None if isinstance(integrator, str) and integrator == 'leapfrog' else _hip.hmc_scheme(integrator)

    def _advance(self, batch_size, n_chains, n_md, dt, n_skip, path, want_rows, want_stats, cluster_every=0,
                 improved=False, integrator='leapfrog', momenta=None, spectrum_path=None, fa_mass_sq=None, modes=None,
                 modes_path=None):
        """batch_size // n_chains recorded steps of the chains: (the rows (batch_size, *L) or None, the `_Stats` of the
        recorded states or None); the chains, `last` and `history` updated.  cluster_every = E >= 1: the recorded steps
        are run in spans that end before the next step s (counted across calls) with s % E == 0, with one cluster sweep
        of all chains in front of each such step; the span's launches are those of a call of that many steps."""
        n_chains, n_md, every, E = self._checked(batch_size, n_chains, n_md, n_skip, cluster_every, 'cluster_every')
        scheme = self._scheme(integrator)
        self._restart(n_chains)
        phi, S = self._ref['sample'], self._ref['action']
        fa = None
        if fa_mass_sq is None:
            path = self._choose(phi, path)
        else:
            path = self._choose_fa(phi, path)
            fa = _Fourier(phi, self._fa_w0(phi), fa_mass_sq)
        rows = batch_size // n_chains
        out = torch.empty((rows,) + tuple(phi.shape), dtype=phi.dtype, device=phi.device) if want_rows else None
        stats = _Stats(phi, rows) if want_stats else None
        ws = self._tiled_workspace(phi) if path == 'tiled' else None       # one workspace for all calls
        if path == 'fa_tiled':
            need = _hip.hmc_fa_tiled_workspace(phi.shape[0], tuple(phi.shape[1:]), phi.dtype)
            ws = torch.empty(max(need, 256), dtype=torch.uint8, device=phi.device)
        sweep_ws = None
        if E and self._sweep_path(phi) == 'tiled':                # one workspace for all sweeps of the call
            need = _hip.cluster_tiled_workspace(phi.shape[0], tuple(phi.shape[1:]))
            sweep_ws = torch.empty(max(need, 256), dtype=torch.uint8, device=phi.device)
        if path != 'composed':
            phi = phi.clone()                                     # the kernels run in place
        if improved is not False:
            from ..lib.observables import ImprovedMeasurement, measure_improved
            spec = self._spectrum_workspace(phi, momenta, spectrum_path)      # one workspace for all sweeps of the call
            if modes is not None:
                spec = dict(spec, modes=modes, **self._modes_workspace(phi, modes, modes_path))
                modes = _hip.modes_reduced(tuple(phi.shape[1:]), modes)       # what an empty measurement carries
        dhs, accs, sweeps, parts, r0 = [], [], [], [], 0
        while r0 < rows:
            if E and (self._steps + r0) % E == 0:
                if improved is False:
                    phi, st = self._sweep(phi, workspace=sweep_ws)
                else:                                                 # the same sweep, its labels kept
                    phi, st, labels = self._sweep(phi, workspace=sweep_ws, want_labels=True)
                    parts.append(measure_improved(phi, labels, path=improved, momenta=momenta, **spec))
                sweeps.append(st)
                if path == 'composed':
                    S = self._model.action(phi.double()).double()
            k = self._span(self._steps + r0, rows - r0, E)
            sink = _Span(out, stats, r0)
            if path == 'composed':
                phi, S = self._run_composed(phi, S, k, every, n_md, dt, sink, dhs, accs, scheme,
                                            **({} if fa is None else dict(fa=fa)))
            elif path == 'fa':
                S = self._run_fa(phi, self._coef(phi.shape[1:]), fa.mass_sq, k, every, n_md, dt, sink, dhs, accs, scheme)
            elif path == 'fa_tiled':
                S = self._run_fa_tiled(phi, self._coef(phi.shape[1:]), fa.mass_sq, k, every, n_md, dt, ws, sink, dhs, accs,
                                       scheme)
            else:
                S = self._run(path, phi, self._coef(phi.shape[1:]), k, every, n_md, dt, ws, sink, dhs, accs, scheme)
            r0 += k
        self._steps += rows
        self._ref.update(sample=phi, action=S)
        self._finish(dhs, accs, scheme=scheme)
        if fa is not None:
            self.last['fa_mass_sq'] = fa.mass_sq
        if path == 'fa_tiled':
            self.last['path'] = path
        if E:
            self.last['cluster'] = (torch.stack(sweeps) if sweeps else
                                    torch.empty((0, phi.shape[0], 4), dtype=torch.int32, device=phi.device))
        if improved is not False:                 # only `measure` asks, so there are stats to carry the rows
            K = None if momenta is None else _hip.spectrum_momenta(tuple(phi.shape[1:]), momenta)
            stats.improved = ImprovedMeasurement.cat(parts, tuple(phi.shape[1:]), phi.device, K, modes)
        y = None if out is None else out.reshape((batch_size,) + tuple(phi.shape[1:]))
        return y, stats

    # ---- what every sampler of this family does around its launches
    @staticmethod
    def _checked(batch_size, n_chains, n_md, n_skip, E, name):
        """(n_chains, n_md, every = n_skip + 1, E) as integers, checked; `name` is the caller's word for E."""
        n_chains, n_md, every, E = int(n_chains), int(n_md), int(n_skip) + 1, int(E)
        if n_chains < 1 or batch_size < 1 or batch_size % n_chains != 0:
            raise ValueError(f"batch_size ({batch_size}) must be a positive multiple of n_chains ({n_chains})")
        if n_md < 1 or every < 1:
            raise ValueError(f"n_md ({n_md}) must be >= 1 and n_skip ({n_skip}) >= 0")
        if E < 0:
            raise ValueError(f"{name} ({E}) must be >= 0")
        return n_chains, n_md, every, E

    def _restart(self, n_chains):
        """Chains from the prior where there are none, or not n_chains of them."""
        s = self._ref['sample']
        if s is None or s.shape[0] != n_chains:
            print("Starting from scratch")
            self.start(n_chains=n_chains)

    @staticmethod
    def _span(done, left, E):
        """The recorded steps of the next span, `done` steps after `start()` with `left` to go: up to the next multiple
        of E (the cluster sweep falls before a span, the exchange sweep after it); E = 0: all of them."""
        return min(left, E - done % E) if E else left

    @staticmethod
    def _tiled_workspace(phi):
        need = _hip.hmc_tiled_workspace(phi.shape[0], tuple(phi.shape[1:]), phi.dtype)
        return torch.empty(max(need, 256), dtype=torch.uint8, device=phi.device)

    def _finish(self, dhs, accs, extra=None, scheme=None):
        """`last` = the call's dH and accept flags (trajectories, C), left on the device, and `history`'s three entries,
        by the call's ONE device-to-host read; the float64 vector `extra` rides in it and comes back as a list.  A
        `scheme` (an integrator other than leapfrog) is recorded as `last['integrator']`."""
        dh, acc = (dhs[0], accs[0]) if len(dhs) == 1 else (torch.cat(dhs), torch.cat(accs))
        self.last = dict(dh=dh, accept=acc)
        if scheme is not None:
            self.last['integrator'] = scheme.label()
        got = torch.stack([acc.double().mean(), torch.exp(-dh).mean(), dh.square().mean().sqrt()])
        got = (got if extra is None else torch.cat([got, extra])).cpu().tolist()
        for key, val in zip(HMCHistory._KEYS, got):
            getattr(self.history, key).append(val)
        return got[len(HMCHistory._KEYS):]

    @torch.no_grad()
    def start(self, phi=None, n_chains=1):
        """Start the chains from phi (C, *L) -- flow samples, say -- or from model.prior.sample(n_chains)."""
        if phi is None:
            phi = self._model.prior.sample(int(n_chains))
        phi = phi.detach().clone().contiguous()
        if phi.dtype not in (torch.float32, torch.float64):
            raise TypeError(f"HMCSampler supports float32 and float64 fields, got {phi.dtype}")
        self._ref.update(sample=phi, action=self._model.action(phi.double()).double())
        self._steps = 0
        return self

    @torch.no_grad()
    def cluster(self, phi, position=None, path=None):
        """ONE Swendsen-Wang sweep of the signs of the chains phi (C, *L), which are left alone; the stored chains are
        not touched.  Returns dict(phi = the swept chains, labels (C, *L) int32 = the smallest site index of every
        site's cluster, stats (C, 4) int32 = clusters, sites flipped, size of the largest cluster, and the count of
        `last['cluster']`: rounds, or the tiles of a chain on the tiled path).  `position` = (seed, offset) fixes the two
        Philox positions of a device sweep instead of taking them from torch's CUDA generator.  `path`: None (the
        sampler's own choice, `_sweep_path`), 'kernel' (nf_phi4_cluster), 'tiled' (nf_phi4_cluster_tiled) or 'composed'
        (`cluster_sweep`, mcmc/cluster.py); a forced path that does not apply raises."""
        new, stats, labels = self._sweep(phi.detach(), position=position, want_labels=True, path=path)
        return dict(phi=new, labels=labels, stats=stats)

    def _sweep_path(self, phi, path=None):
        """'kernel', 'tiled' or 'composed'.  None: nf_phi4_cluster wherever it takes the chains (it beats the composed
        sweep on every class measured, README); else nf_phi4_cluster_tiled on the classes of cluster.TILED_CLASSES
        (3 or 4 axes of extent > 1, from the smallest lattice of that many axes on which tools/cluster_bench.py --tiled
        measured it faster than the composed sweep by more than the margin); else composed.  The kernels take a ScalarPhi4Action on a HIP device."""
        from .cluster import PATHS, TILED_CLASSES
        if path not in PATHS:
            raise ValueError(f"path must be None, 'kernel', 'tiled' or 'composed', got {path!r}")
        if path == 'composed':
            return path
        lat = tuple(phi.shape[1:])
        on_device = phi.is_cuda and isinstance(self._model.action, ScalarPhi4Action)
        if path != 'tiled' and on_device and _hip.cluster_supported(lat, phi.dtype):
            return 'kernel'
        tiled = on_device and _hip.cluster_tiled_supported(lat, phi.dtype)
        if path is None:
            V, axes = phi[0].numel(), sum(1 for n in lat if n > 1)
            measured = any(phi.dtype == dt and axes == d and V >= least for dt, d, least in TILED_CLASSES)
            return 'tiled' if tiled and measured else 'composed'
        if path == 'tiled' and tiled:
            return path
        raise _hip.NormflowHipError(
            f"HMCSampler.cluster(path={path!r}): nf_phi4_cluster{'_tiled' if path == 'tiled' else ''} does not apply to a "
            f"{type(self._model.action).__name__} and a {phi.device} tensor of shape {lat} and {phi.dtype}")

    def _sweep_couplings(self, phi):
        """What a sweep of the chains phi takes after them: (w0,); the ladder's sampler gives (coef, rung)."""
        action = self._model.action
        if not hasattr(action, 'get_coef'):
            raise TypeError("cluster sweeps need the hopping coefficient of a phi^4 action (get_coef), got a "
                            f"{type(action).__name__}")
        return (float(action.get_coef(phi.ndim - 1)[0]),)

    def _sweep(self, phi, position=None, want_labels=False, path=None, workspace=None, couplings=None):
        """(the swept copy of phi, stats[, labels]) by the path `_sweep_path` names: a kernel, or composed -- on the device
        with the kernel's draws from the same two positions, on CPU tensors with torch's CPU generator.  `workspace`: the
        tiled kernel's, when the caller keeps one for several sweeps.  `couplings`: `_sweep_couplings(phi)` unless given;
        the pair (coef, rung) goes to the ladder kernels as it is and to the composed sweep as coef[rung, 0]."""
        couplings = self._sweep_couplings(phi) if couplings is None else couplings
        ladder = len(couplings) == 2
        lat = tuple(phi.shape[1:])
        path = self._sweep_path(phi, path)
        if path != 'composed':
            new = phi.clone().contiguous()
            kernel = getattr(_hip, 'phi4_cluster' + ('_tiled' if path == 'tiled' else '') + ('_ladder' if ladder else ''))
            kw = dict(workspace=workspace) if path == 'tiled' else {}
            r = kernel(new, *couplings, position=position, want_labels=want_labels, **kw)
            return (new, r['stats'], r['labels']) if want_labels else (new, r['stats'])
        from .cluster import cluster_sweep
        # a chain's rung clamped into the table, as the kernels clamp it
        w0 = couplings[0][couplings[1].long().clamp(0, couplings[0].shape[0] - 1), 0] if ladder else couplings[0]
        C, V = phi.shape[0], phi[0].numel()
        if phi.is_cuda:
            u, flip = _hip.phi4_cluster_draws(C, lat, phi.device, position=position)
        else:
            u = torch.rand((C, V, 4), dtype=torch.float64, device=phi.device)
            flip = torch.rand((C, V), dtype=torch.float64, device=phi.device) < 0.5
        new, labels, stats = cluster_sweep(phi, w0, u, flip)
        return (new, stats, labels) if want_labels else (new, stats)

    @torch.no_grad()
    def trajectory(self, phi, n_md=10, dt=0.1, pi=None, force_accept=False, path=None, position=None,
                   integrator='leapfrog', fa_mass_sq=None):
        """ONE trajectory of the chains phi (C, *L), which are left alone; the stored chains are not touched.  Returns
        dict(phi = the states after the decision, pi = the momenta at the end of the trajectory, dh (C) float64,
        accept (C) uint8, action (C) float64 = S of the returned states).  `pi` replaces the drawn momenta.  `position`
        = (seed, offset) fixes the Philox position of a device run instead of taking it from torch's CUDA generator.
        `integrator` and `fa_mass_sq` as in `sample_`; with fa_mass_sq, `pi` (in and out) is pi, not the drawn eta."""
        phi = phi.detach().clone().contiguous()
        scheme = self._scheme(integrator)
        fa = None
        if fa_mass_sq is None:
            path = self._choose(phi, path)
        else:
            path = self._choose_fa(phi, path)
            fa = _Fourier(phi, self._fa_w0(phi), fa_mass_sq)
        if path in ('fa', 'fa_tiled'):
            kw = {} if scheme is None else dict(scheme=scheme)
            kernel = _hip.phi4_hmc_fa if path == 'fa' else _hip.phi4_hmc_fa_tiled
            r = kernel(phi, *self._coef(phi.shape[1:]), n_md, dt, fa.mass_sq, n_traj=1, pi_in=pi, want_pi=True,
                       force_accept=force_accept, position=position, **kw)
            return dict(phi=phi, pi=r['pi'], dh=r['dh'][0], accept=r['accept'][0], action=r['action'])
        if path != 'composed':
            kernel = _hip.phi4_hmc if path == 'fused' else _hip.phi4_hmc_tiled
            kw = {} if scheme is None else dict(scheme=scheme)
            r = kernel(phi, *self._coef(phi.shape[1:]), n_md, dt, n_traj=1, pi_in=pi, want_pi=True,
                       force_accept=force_accept, position=position, **kw)
            return dict(phi=phi, pi=r['pi'], dh=r['dh'][0], accept=r['accept'][0], action=r['action'])
        gen = None
        if position is not None:
            gen = torch.Generator(device=phi.device)
            gen.manual_seed(position[0])
            gen.set_offset(4 * position[1])
        S0 = self._model.action(phi.double()).double()
        phi, S, dh, acc, pi = self._trajectory_composed(phi, S0, n_md, dt, pi=pi, force_accept=force_accept, generator=gen,
                                                        scheme=scheme, **({} if fa is None else dict(fa=fa)))
        return dict(phi=phi, pi=pi, dh=dh, accept=acc, action=S)

    def ladder(self, ladder):
        """The sampler of the coupling ladder `ladder` (a ScalarPhi4Ladder) with this model's prior: per-chain couplings in
        one launch and replica exchange between neighbouring rungs (mcmc/ladder.py)."""
        from .ladder import LadderHMCSampler
        return LadderHMCSampler(self._model, ladder)

    # ---- which path
    def _fused_applies(self, phi):
        return (isinstance(self._model.action, ScalarPhi4Action) and phi.is_cuda
                and _hip.hmc_supported(tuple(phi.shape[1:]), phi.dtype))

    def _tiled_refusal(self, phi):
        """Why nf_phi4_hmc_tiled does not take these chains, or None."""
        if not isinstance(self._model.action, ScalarPhi4Action):
            return f"the action is a {type(self._model.action).__name__}, not a ScalarPhi4Action"
        if not phi.is_cuda:
            return f"the chains are a {phi.device} tensor, not on a HIP device"
        if phi.dtype not in (torch.float32, torch.float64):
            return f"the chains are {phi.dtype}, not float32 or float64"
        if not _hip.hmc_tiled_supported(tuple(phi.shape[1:]), phi.dtype):
            return f"the lattice {tuple(phi.shape[1:])} has more than four axes or 2^31 sites or more"
        return None

    def _choose(self, phi, path):
        """'fused', 'tiled' or 'composed'."""
        if path not in (None, 'fused', 'tiled', 'composed'):
            raise ValueError(f"path must be None, 'fused', 'tiled' or 'composed', got {path!r}")
        if path == 'composed':
            return path
        if path == 'tiled':
            why = self._tiled_refusal(phi)
            if why is not None:
                raise _hip.NormflowHipError(f"HMCSampler(path='tiled'): nf_phi4_hmc_tiled does not apply: {why}")
            return path
        if self._fused_applies(phi):
            return 'fused'
        if path == 'fused':
            raise _hip.NormflowHipError(
                "HMCSampler(path='fused'): nf_phi4_hmc takes a ScalarPhi4Action on a HIP device and a lattice whose chain "
                f"fits its LDS image; got {type(self._model.action).__name__}, a {phi.device} tensor of shape "
                f"{tuple(phi.shape[1:])} and {phi.dtype}")
        return 'tiled' if self._tiled_refusal(phi) is None else 'composed'

    def _fa_w0(self, phi):
        """The hopping coefficient that a(k) is built from."""
        action = self._model.action
        if not hasattr(action, 'get_coef'):
            raise TypeError("Fourier acceleration builds a(k) from the hopping coefficient of a phi^4 action (get_coef), "
                            f"got a {type(action).__name__}")
        return float(action.get_coef(phi.ndim - 1)[0])

    def _fa_refusal(self, phi):
        """Why nf_phi4_hmc_fa does not take these chains, or None."""
        if not isinstance(self._model.action, ScalarPhi4Action):
            return f"the action is a {type(self._model.action).__name__}, not a ScalarPhi4Action"
        if not phi.is_cuda:
            return f"the chains are a {phi.device} tensor, not on a HIP device"
        if not _hip.hmc_fa_supported(tuple(phi.shape[1:]), phi.dtype):
            return (_hip.last_error() if phi.dtype in (torch.float32, torch.float64) and 1 <= phi.ndim - 1 <= 4
                    else f"the chains are {phi.dtype} on {phi.ndim - 1} axes")
        return None

    def _fa_tiled_refusal(self, phi):
        """Why nf_phi4_hmc_fa_tiled does not take these chains, or None: the planner's reason where it is the planner's."""
        if not isinstance(self._model.action, ScalarPhi4Action):
            return f"the action is a {type(self._model.action).__name__}, not a ScalarPhi4Action"
        if not phi.is_cuda:
            return f"the chains are a {phi.device} tensor, not on a HIP device"
        if not _hip.hmc_fa_tiled_supported(tuple(phi.shape[1:]), phi.dtype):
            return (_hip.last_error() if phi.dtype in (torch.float32, torch.float64) and 1 <= phi.ndim - 1 <= 4
                    else f"the chains are {phi.dtype} on {phi.ndim - 1} axes")
        return None

    def _choose_fa(self, phi, path):
        """'fa', 'fa_tiled' or 'composed', with fa_mass_sq: None is the kernel where nf_phi4_hmc_fa_supported holds on device
        tensors and the composed path everywhere else; the accelerated kernel for chains in HBM (nf_phi4_hmc_fa_tiled, the
        lattices beyond one CU) runs only where `path='fa_tiled'` asks for it."""
        if path in ('tiled', 'fused'):
            raise ValueError(f"path={path!r} with fa_mass_sq: there is no {path} accelerated kernel under that name (lattices "
                             "beyond one CU run the composed path, or nf_phi4_hmc_fa_tiled with path='fa_tiled'); path must "
                             "be None, 'fa', 'fa_tiled' or 'composed'")
        if path not in (None, 'fa', 'fa_tiled', 'composed'):
            raise ValueError(f"path must be None, 'fa', 'fa_tiled' or 'composed' with fa_mass_sq, got {path!r}")
        if path == 'composed':
            return path
        if path == 'fa_tiled':
            why = self._fa_tiled_refusal(phi)
            if why is not None:
                raise _hip.NormflowHipError(f"HMCSampler(path='fa_tiled'): nf_phi4_hmc_fa_tiled does not apply: {why}")
            return path
        why = self._fa_refusal(phi)
        if why is None:
            return 'fa'
        if path == 'fa':
            raise _hip.NormflowHipError(f"HMCSampler(path='fa'): nf_phi4_hmc_fa does not apply: {why}")
        return 'composed'

    def _coef(self, lat):
        """(w0, w2, w4) as nf_phi4_hmc takes them: ScalarPhi4Action.action's rule for a user axis of extent 1 (it is its own
        neighbour: -w0 phi^2) folded into w2, as for nf_phi4_action."""
        w0, w2, w4 = self._model.action.get_coef(len(lat))
        own = sum(1 for n in lat if n == 1)
        return float(w0), float(w2 - own * w0), float(w4)

    # ---- fused and tiled
    def _run(self, path, phi, couplings, rows, every, n_md, dt, ws, sink, dhs, accs, scheme=None):
        """`rows` recorded steps of the chains phi, IN PLACE, by the kernel of `path`, in the launches that `schedule`
        (mcmc/schedule.py) cuts them into under the kernel's work cap (`_hip.hmc_fused_budget`, `_hip.hmc_tiled_budget`).
        `couplings`: (w0, w2, w4), or the ladder kernels' (coef, rung).  Rows and statistics go to `sink` (a `_Span`), dH
        and the accept flags of every launch to the lists.  Returns S (C) of the chains.  `scheme` (None: leapfrog, and
        the calls as they always were): the caps count force evaluations, so the budget and the schedule are fed
        n_md * s, and every launch gets the scheme."""
        tiled, ladder = path == 'tiled', len(couplings) == 2
        kernel = getattr(_hip, 'phi4_hmc' + ('_tiled' if tiled else '') + ('_ladder' if ladder else ''))
        evals = n_md * (1 if scheme is None else scheme.stages)
        extra = {} if scheme is None else dict(scheme=scheme)
        budget = _hip.hmc_tiled_budget(evals) if tiled else _hip.hmc_fused_budget(phi[0].numel(), phi.shape[0])
        for a in schedule(rows, every, evals, budget, tiled=tiled, ladder=ladder, stats=sink.stats is not None,
                          want_rows=sink.out is not None, measure_cost=_hip.HMC_MEASURE_MD_STEPS):
            if isinstance(a, Take):
                sink.take(a.row, phi, a.copy)
                continue
            kw = dict(workspace=ws) if tiled else dict(measure=a.measure, record=a.record)
            r = kernel(phi, *couplings, n_md, dt, n_traj=a.n_traj, record_every=a.record_every, **kw, **extra)
            dhs.append(r['dh']); accs.append(r['accept'])
            sink.launch(a.row0, r)
        return r['action']

    # ---- Fourier-accelerated kernel
    def _run_fa(self, phi, couplings, mass_sq, rows, every, n_md, dt, sink, dhs, accs, scheme=None):
        """`_run` for nf_phi4_hmc_fa, by `schedule_fa`: the kernel does not measure, so where statistics are wanted its
        launches record the rows and they are measured afterwards, row by row, as `model.measure` would."""
        evals = n_md * (1 if scheme is None else scheme.stages)
        extra = {} if scheme is None else dict(scheme=scheme)
        budget = _hip.hmc_fused_budget(phi[0].numel(), phi.shape[0])
        for a in schedule_fa(rows, every, _hip.hmc_fa_cost(evals), budget, want_rows=sink.out is not None,
                             stats=sink.stats is not None):
            if isinstance(a, Take):
                sink.take(a.row, phi, a.copy)
                continue
            r = _hip.phi4_hmc_fa(phi, *couplings, n_md, dt, mass_sq, n_traj=a.n_traj, record_every=a.record_every,
                                 record=a.record, **extra)
            dhs.append(r['dh']); accs.append(r['accept'])
            if r['record'] is not None:
                if sink.out is not None:
                    sink.launch(a.row0, r)
                if sink.stats is not None:
                    for i in range(r['record'].shape[0]):
                        sink.put_stats(a.row0 + i, r['record'][i])
        return r['action']

    # ---- Fourier-accelerated kernel, chains in HBM
    def _run_fa_tiled(self, phi, couplings, mass_sq, rows, every, n_md, dt, ws, sink, dhs, accs, scheme=None):
        """`_run`'s tiled route for nf_phi4_hmc_fa_tiled: the launches that `schedule(tiled=True)` cuts under
        `_hip.hmc_fa_tiled_budget`, one workspace, the statistics taken from the chains in place between the launches."""
        evals = n_md * (1 if scheme is None else scheme.stages)
        extra = {} if scheme is None else dict(scheme=scheme)
        passes = _hip.hmc_fa_tiled_plan(tuple(phi.shape[1:]), phi.dtype)['passes']
        budget = _hip.hmc_fa_tiled_budget(evals, passes)
        for a in schedule(rows, every, evals, budget, tiled=True, ladder=False, stats=sink.stats is not None,
                          want_rows=sink.out is not None, measure_cost=_hip.HMC_MEASURE_MD_STEPS):
            if isinstance(a, Take):
                sink.take(a.row, phi, a.copy)
                continue
            r = _hip.phi4_hmc_fa_tiled(phi, *couplings, n_md, dt, mass_sq, n_traj=a.n_traj, record_every=a.record_every,
                                       workspace=ws, **extra)
            dhs.append(r['dh']); accs.append(r['accept'])
            sink.launch(a.row0, r)
        return r['action']

    # ---- composed
    def _force(self, phi):
        with torch.enable_grad():
            p = phi.detach().requires_grad_(True)
            (F,) = torch.autograd.grad(self._model.action(p).sum(), p)
        return F

    def _energy(self, phi, pi):
        return 0.5 * pi.double().square().flatten(1).sum(dim=1) + self._model.action(phi.double()).double()

    def _trajectory_composed(self, phi, S0, n_md, dt, pi=None, force_accept=False, generator=None, scheme=None, fa=None):
        """One trajectory by the definition at the top of the module; the update lengths are the doubles a_j dt, b_j dt
        and 0.5 b_s dt, as the kernels are handed them (leapfrog: dt and 0.5 dt).  `fa` (a `_Fourier`): the accelerated
        rule -- the drawn eta becomes pi = A^(-1/2) eta, the kinetic energy is sum pi (A pi) / 2 and phi moves by A pi."""
        kinetic = (lambda p: 0.5 * p.double().square().flatten(1).sum(dim=1)) if fa is None else fa.kinetic
        velocity = (lambda p: p) if fa is None else fa.apply
        a, b = ((1.0,), (1.0,)) if scheme is None else (scheme.a, scheme.b)
        s, half = len(a), 0.5 * b[-1] * dt
        C, shape = phi.shape[0], tuple(phi.shape[1:])
        on_device = phi.is_cuda
        if pi is None:
            if on_device:
                pi = _hip.normal_sample(None, None, C, shape, phi.dtype, phi.device, generator=generator)[0]
            else:
                pi = torch.randn(phi.shape, dtype=phi.dtype, device=phi.device)
            if fa is not None:
                pi = fa.refresh(pi)
        elif on_device:
            _hip._philox_position(phi.device, generator)      # handed-in momenta still take the position of the draw
        H0 = kinetic(pi) + S0
        new = phi
        pi = pi - half * self._force(new)
        for k in range(1, n_md + 1):
            for j in range(s):
                new = new + (a[j] * dt) * velocity(pi)
                pi = pi - (half if k == n_md and j == s - 1 else b[j] * dt) * self._force(new)
        S1 = self._model.action(new.double()).double()
        dh = kinetic(pi) + S1 - H0
        if on_device:
            new = new.contiguous()
            acc = torch.empty(C, dtype=torch.uint8, device=phi.device)
            # the whole field as one block: accept iff log u < 0 - (dH - 0); the kernel restores the rejected chains
            _hip.block_accept(new, phi.reshape(C, -1).contiguous(), dh.to(phi.dtype), torch.zeros(C, dtype=phi.dtype, device=phi.device),
                              torch.zeros(C, dtype=torch.float64, device=phi.device), acc, new[0].numel(), 0,
                              force_accept=force_accept, generator=generator)
            ok = acc.bool()
        else:
            logu = torch.log(1.0 - torch.rand(C, dtype=torch.float64, device=phi.device))       # u in (0, 1]
            ok = (logu < -dh) | bool(force_accept)
            new = torch.where(ok.reshape((C,) + (1,) * len(shape)), new, phi)
            acc = ok.to(torch.uint8)
        return new, torch.where(ok, S1, S0), dh, acc, pi

    def _run_composed(self, phi, S, rows, every, n_md, dt, sink, dhs, accs, scheme=None, **fa):
        for t in range(rows * every):
            phi, S, dh, acc, _ = self._trajectory_composed(phi, S, n_md, dt, scheme=scheme, **fa)
            dhs.append(dh.unsqueeze(0)); accs.append(acc.unsqueeze(0))
            if (t + 1) % every == 0:
                sink.take((t + 1) // every - 1, phi)
        return phi, S


class _Fourier:
    """The kinetic operator of the accelerated rule on the lattice of the chains phi (C, *L), from torch ops: a(k) and
    a^(-1/2)(k) from the shared table (`_hip.hmc_fa_denominator`), formed in double and cast to the field dtype, and the
    filter T diag(d) T x = irfftn(rfftn(x) d) (d is even in every k_mu, so its half along the last axis is all rfftn
    needs)."""

    def __init__(self, phi, w0, mass_sq):
        mass_sq = float(mass_sq)
        if not mass_sq > 0.0 or mass_sq == float('inf'):
            raise ValueError(f"fa_mass_sq must be a finite number > 0, got {mass_sq}")
        if w0 < 0.0:
            raise ValueError(f"Fourier acceleration needs a hopping coefficient w0 >= 0 (a(k) > 0), got {w0}")
        self.mass_sq = mass_sq
        self.lat = tuple(phi.shape[1:])
        self.axes = tuple(range(1, phi.ndim))
        den = _hip.hmc_fa_denominator(self.lat, w0, mass_sq)
        nh = self.lat[-1] // 2 + 1
        self.a = (1.0 / den)[..., :nh].to(phi.dtype).to(phi.device)
        self.inv_sqrt_a = den.sqrt()[..., :nh].to(phi.dtype).to(phi.device)

    def _filter(self, x, d):
        return torch.fft.irfftn(torch.fft.rfftn(x, dim=self.axes) * d, s=self.lat, dim=self.axes)

    def apply(self, pi):
        """A pi."""
        return self._filter(pi, self.a)

    def refresh(self, eta):
        """pi = A^(-1/2) eta."""
        return self._filter(eta, self.inv_sqrt_a)

    def kinetic(self, pi):
        """sum pi (A pi) / 2 per chain, in double."""
        return 0.5 * (pi.double() * self.apply(pi).double()).flatten(1).sum(dim=1)


class _Stats:
    """The statistics of `rows` recorded steps of the chains phi (C, *L), gathered step by step, as
    `observables.measure` takes them from the stored rows: by the kernel that `observables.route` names for the chains
    (its rows do not depend on how many are measured at once), else by the composed sums."""

    def __init__(self, phi, rows):
        from ..lib import observables
        self._ob = observables
        self.lattice = tuple(phi.shape[1:])
        self.path = observables.route(phi)
        self.kernel = None
        self.improved = None            # the call's ImprovedMeasurement, where `measure(improved=...)` asked for one
        if self.path != 'composed':
            self.kernel = _hip.lattice_measure if self.path == 'kernel' else _hip.lattice_measure_tiled
            self.out = torch.empty((rows, phi.shape[0], _hip.measure_n_out(self.lattice)), dtype=torch.float64, device=phi.device)
        else:
            self.parts = [None] * rows

    def put(self, r, phi):
        """Step r: the chains as they lie."""
        if self.kernel is not None:
            self.kernel(phi.contiguous(), out=self.out[r])
        else:
            self.parts[r] = self._ob._compose(phi)

    def put_rows(self, r0, block):
        """Steps r0 ..: (k, C, n_out) rows taken by nf_phi4_hmc_measure."""
        if self.kernel is None:
            raise _hip.NormflowHipError("HMCSampler.measure: the fused kernel's rows are nf_lattice_measure's, which "
                                        f"`observables.route` does not name for the lattice {self.lattice}")
        self.out[r0:r0 + block.shape[0]] = block

    def measurement(self, action=None):
        if self.kernel is not None:
            scalars, links, slices = self._ob._split(self.out.flatten(0, 1), self.lattice)
        else:
            scalars = torch.cat([p[0] for p in self.parts])
            links = torch.cat([p[1] for p in self.parts])
            slices = [torch.cat([p[2][mu] for p in self.parts]) for mu in range(len(self.lattice))]
        return self._ob.Measurement(scalars, links, slices, self.lattice, action)


class _Span:
    """What the recorded steps first .. of a call, numbered from 0, write into: the call's rows `out` and its statistics
    `stats` (a `_Stats`; the ladder's `_RungStats`), either of them None where not wanted.  `col`: the chains hold rungs,
    and a row taken from the chains is laid out by the column `col` of every chain."""

    def __init__(self, out, stats, first, col=None):
        self.out, self.stats, self._first, self._col = out, stats, first, col

    def launch(self, r0, r):
        """Steps r0 ..: what the launch with the dict r recorded and measured, if it did."""
        r0 += self._first
        if r['record'] is not None:
            self.out[r0:r0 + r['record'].shape[0]] = r['record']
        if 'measure' in r:
            self.stats.put_rows(r0, r['measure'])

    def put_stats(self, r, phi):
        """Step r: the statistics of the recorded row phi (C, *L)."""
        self.stats.put(r + self._first, phi)

    def take(self, r, phi, copy=True):
        """Step r from the chains as they lie: its statistics, and the row itself unless a launch recorded it."""
        r += self._first
        if copy and self.out is not None:
            if self._col is None:
                self.out[r] = phi
            else:
                self.out[r].index_copy_(0, self._col, phi)
        if self.stats is not None:
            self.stats.put(r, phi)
