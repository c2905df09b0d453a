"""What the samplers' rows measure (MI355X-side extension; the reference stops at `Resampler` and `estimate_logz`).

`measure(cfgs)` reduces every configuration (N, *L), 1 <= d <= 4, to its sufficient statistics in double -- on the device
in ONE pass of the `nf_lattice_measure` kernel or, for rows beyond it, of the brick-tiled `nf_lattice_measure_tiled`
(include/normflow_hip.h; `route` says which), on host tensors by the same definitions composed from torch ops:
    sum_phi, sum_phi2, sum_phi4      sum_x phi, phi^2, phi^4
    links[:, mu]                     sum_x phi(x) phi(x - mu), periodic; 0 along an axis of extent 1
    slices[mu][:, t]                 S_mu(t) = sum over the sites with x_mu = t of phi(x)
Everything else is O(N sum L) host arithmetic on those: the action, the magnetisation m = sum phi / V and its moments, the
time-slice correlator
    G_mu(t) = (1 / L_mu) sum_s pbar_mu(s) pbar_mu(s + t),   pbar_mu = S_mu / (V / L_mu),
and the on-axis momentum-space propagator |sum_t e^{ipt} S_mu(t)|^2 / V at p = 2 pi k / L_mu.

`measure_improved(cfgs, labels)` gives the cluster-improved forms of (sum phi)^2, (sum phi)^4 and the propagator at
p_min from the labels of a Swendsen-Wang sweep (`ImprovedMeasurement`, `ImprovedEnsemble`; nf_cluster_moments on the
device).  With `momenta='all'` it also carries the cluster spectrum (nf_cluster_spectrum), from which the improved
propagator at every on-axis momentum and the improved time-slice correlator follow; `spectrum_path='hbm'` takes it with
nf_cluster_spectrum_tiled, the kernel for lattices beyond one CU's LDS.  With `modes=[(n0, ...), ...]` it carries the
same sums at a list of momentum vectors, on or off the axes (nf_cluster_modes): `mode_propagator`, `mode_correlator` at a
spatial momentum, and through `measure_modes(cfgs, modes)` the plain |phi~(p)|^2 from the same kernel;
`modes_path='hbm'` takes them with nf_cluster_modes_tiled, the kernel for lattices beyond one CU's LDS.

`Ensemble` reads the rows as (steps, chains) -- row r = step r // C of chain r % C, the layout of model.mcmc,
model.blocked_mcmc and model.hmc -- and gives every estimate as (value, error): leave-one-chain-out jackknife for
C >= 2, binned jackknife (`Resampler('jackknife')`) for one chain; `tau_int` is the integrated autocorrelation time with
the Madras-Sokal window."""
import math

import torch

from .. import _hip
from .stats import Resampler

# the regimes of nf_lattice_measure_plan on which `measure` runs the kernel: those where tools/measure_bench.py measured
# it no slower than the composed path on an MI355X (README, "Observables")
KERNEL_REGIMES = ('packed', 'resident', 'segmented')
# (dtype, least bytes of a row): the classes that nf_lattice_measure refuses and on which tools/measure_bench.py measured
# the brick-tiled kernel faster than the composed path by its margin on an MI355X -- 32^4 in fp64, 48^4 in both dtypes
# (README, "Observables").  `route` sends only these to it; a refused lattice outside them stays composed until measured
TILED_CLASSES = ((torch.float64, 32 ** 4 * 8), (torch.float32, 48 ** 4 * 4))
PATHS = (None, 'kernel', 'tiled', 'composed')


def _compose(x):
    """The statistics of (N, *L) rows from torch ops in double: d + 3 passes.  Returns (scalars (N, 3), links (N, d),
    slices: list of (N, L_mu))."""
    x = x.double()
    d = x.ndim - 1
    sq = x * x
    tot = lambda t: t.flatten(1).sum(1)
    scalars = torch.stack([tot(x), tot(sq), tot(sq * sq)], dim=1)
    links = [tot(x * x.roll(1, dims=mu)) if x.shape[mu] > 1 else torch.zeros_like(scalars[:, 0]) for mu in range(1, d + 1)]
    slices = [x.sum(dim=[nu for nu in range(1, d + 1) if nu != mu]) if d > 1 else x for mu in range(1, d + 1)]
    return scalars, torch.stack(links, dim=1), slices


def _split(out, lat):
    """The (N, 7 + sum of the padded extents) rows of either kernel as `_compose` returns them (views of `out`)."""
    pad = 4 - len(lat)
    at, slices = 7 + pad, []
    for n in lat:
        slices.append(out[:, at:at + n])
        at += n
    return out[:, :3], out[:, 3 + pad:7], slices


def _on_device(cfgs):
    return cfgs.is_cuda and cfgs.dtype in (torch.float32, torch.float64) and cfgs.shape[0] > 0 and 1 <= cfgs.ndim - 1 <= 4


def kernel_applies(cfgs):
    """True where `measure` runs nf_lattice_measure: fp32 / fp64 rows on the device, on a lattice the launcher's planner
    takes, in a regime of KERNEL_REGIMES."""
    lat = tuple(cfgs.shape[1:])
    if not (cfgs.is_cuda and cfgs.dtype in (torch.float32, torch.float64) and cfgs.shape[0] > 0):
        return False
    return _hip.measure_supported(lat, cfgs.dtype) and _hip.measure_plan(lat, cfgs.dtype)['regime'] in KERNEL_REGIMES


def tiled_applies(cfgs):
    """True where `measure(cfgs, path='tiled')` can run nf_lattice_measure_tiled: fp32 / fp64 rows on the device, on a
    lattice its planner takes at the default cap.  Where `measure` takes it unasked is `route`'s matter."""
    return bool(_on_device(cfgs) and _hip.measure_tiled_supported(tuple(cfgs.shape[1:]), cfgs.dtype))


def route(cfgs):
    """The path that `measure(cfgs)` takes: 'kernel' wherever `kernel_applies` (unchanged by the tiled kernel), 'tiled'
    where only the brick-tiled kernel applies and the row falls into one of TILED_CLASSES, else 'composed'."""
    if not _on_device(cfgs):
        return 'composed'
    if kernel_applies(cfgs):
        return 'kernel'
    row_bytes = math.prod(cfgs.shape[1:]) * cfgs.element_size()
    if tiled_applies(cfgs) and any(cfgs.dtype == dt and row_bytes >= least for dt, least in TILED_CLASSES):
        return 'tiled'
    return 'composed'


@torch.no_grad()
def measure(cfgs, action=None, path=None):
    """(N, *L) configurations -> `Measurement`.  path=None: what `route` says -- the kernel where `kernel_applies`, the
    brick-tiled kernel on the classes of large rows where it was measured faster, else the composed torch path (host
    tensors, other dtypes, lattices no kernel takes); 'kernel' / 'tiled' / 'composed' force one (a kernel that cannot run
    raises).  With a `ScalarPhi4Action` the measurement also carries the action of every row; any other action object
    is a TypeError (its action does not follow from these statistics)."""
    if path not in PATHS:
        raise ValueError(f"path must be None, 'kernel', 'tiled' or 'composed', got {path!r}")
    d = cfgs.ndim - 1
    if not 1 <= d <= 4:
        raise ValueError(f"measure: configurations (N, *L) with 1 to 4 lattice axes, got {tuple(cfgs.shape)}")
    lat = tuple(cfgs.shape[1:])
    if path is None:
        path = route(cfgs)
    if path in ('kernel', 'tiled'):
        out = (_hip.lattice_measure if path == 'kernel' else _hip.lattice_measure_tiled)(cfgs.contiguous())
        scalars, links, slices = _split(out, lat)
    else:
        scalars, links, slices = _compose(cfgs)
    return Measurement(scalars, links, slices, lat, action)


class Measurement:
    """Per-row statistics of N configurations, all float64: sum_phi, sum_phi2, sum_phi4 (N), links (N, d), slices (list of
    d tensors (N, L_mu)), volume, lattice, and `action` (N) when made with a ScalarPhi4Action (else None).  `improved`:
    the `ImprovedMeasurement` of the call's cluster sweeps where a sampler's `measure(improved=...)` took one."""

    improved = None

    def __init__(self, scalars, links, slices, lattice, action=None):
        self.sum_phi, self.sum_phi2, self.sum_phi4 = scalars[:, 0], scalars[:, 1], scalars[:, 2]
        self.links, self.slices, self.lattice = links, list(slices), tuple(lattice)
        self.volume = math.prod(self.lattice)
        self.action = None
        if action is not None:
            if not hasattr(action, 'get_coef'):
                raise TypeError(f"a Measurement derives the action of a ScalarPhi4Action (get_coef) from its sums, not of "
                                f"{type(action).__name__}: measure without it")
            w0, w2, w4 = action.get_coef(len(self.lattice))
            own = sum(1 for n in self.lattice if n == 1)          # an axis of extent 1 is its own neighbour
            self.action = (w2 - own * w0) * self.sum_phi2 + w4 * self.sum_phi4 - w0 * links.sum(dim=1)

    def __len__(self):
        return self.sum_phi.shape[0]

    def magnetization(self):
        return self.sum_phi / self.volume

    def phi2(self):
        return self.sum_phi2 / self.volume

    def _axes(self, axis):
        if axis is not None:
            return [range(len(self.lattice))[axis]]
        if len(set(self.lattice)) != 1:
            raise ValueError(f"axis=None averages the axes, whose extents differ on the lattice {self.lattice}: name an axis")
        return list(range(len(self.lattice)))

    def correlator(self, axis=None):
        """(N, L) time-slice correlator G_mu(t), t = 0 .. L - 1, of every row; axis=None: the mean over the axes."""
        out = 0
        for mu in self._axes(axis):
            L = self.lattice[mu]
            f = torch.fft.rfft(self.slices[mu] * (L / self.volume), dim=1)
            out = out + torch.fft.irfft(f.real ** 2 + f.imag ** 2, n=L, dim=1) / L
        return out / len(self._axes(axis))

    def propagator(self, axis=None):
        """(N, L) |sum_t e^{ipt} S_mu(t)|^2 / V at the on-axis momenta p = 2 pi k / L, k = 0 .. L - 1."""
        out = 0
        for mu in self._axes(axis):
            f = torch.fft.fft(self.slices[mu], dim=1)
            out = out + (f.real ** 2 + f.imag ** 2) / self.volume
        return out / len(self._axes(axis))


class Ensemble:
    """Estimates with errors from a `Measurement` of sampler rows: (steps, n_chains) rows, the first `drop` steps left out."""

    NAMES = ('magnetization', 'abs_magnetization', 'm2', 'm4', 'phi2', 'sum_phi', 'sum_phi2', 'sum_phi4', 'action')

    def __init__(self, measurement, n_chains=1, drop=0):
        n = len(measurement)
        if n_chains < 1 or n % n_chains:
            raise ValueError(f"{n} rows are no whole number of steps of {n_chains} chains")
        self.m, self.n_chains, self.drop = measurement, int(n_chains), int(drop)
        self.steps = n // n_chains - self.drop
        if self.steps < 1:
            raise ValueError(f"drop={drop} leaves no step of {n // n_chains}")
        self.volume, self.lattice = measurement.volume, measurement.lattice

    def series(self, name):
        """The per-row quantity `name` (or any (N, ...) tensor) as (steps, chains, K) on the host."""
        if torch.is_tensor(name):
            t = name
        elif name not in self.NAMES:
            raise ValueError(f"unknown observable {name!r}: one of {self.NAMES}")
        else:
            mag = self.m.magnetization()
            t = {'magnetization': mag, 'abs_magnetization': mag.abs(), 'm2': mag ** 2, 'm4': mag ** 4,
                 'phi2': self.m.phi2(), 'sum_phi': self.m.sum_phi, 'sum_phi2': self.m.sum_phi2,
                 'sum_phi4': self.m.sum_phi4, 'action': self.m.action}[name]
            if t is None:
                raise ValueError("the measurement carries no action: measure(cfgs, action)")
        t = t.detach().double().cpu()
        return t.reshape(self.steps + self.drop, self.n_chains, -1)[self.drop:]

    def estimate(self, primaries, fn=lambda mean: mean, binsize=1):
        """(value, error) of fn(<primaries>): primaries (steps, chains, K), fn maps (..., K) means to (..., R).  C >= 2:
        leave-one-chain-out jackknife of the chains' means; C = 1: jackknife over bins of `binsize` steps."""
        C = self.n_chains
        value = fn(primaries.mean(dim=(0, 1)))
        if C >= 2:
            per_chain = primaries.mean(dim=0)
            theta = fn((per_chain.sum(dim=0, keepdim=True) - per_chain) / (C - 1))
            n = C
        else:
            theta = torch.stack([fn(r.mean(dim=0)) for r in Resampler('jackknife')(primaries[:, 0], binsize=binsize)])
            n = theta.shape[0]
        err = ((theta - theta.mean(dim=0)) ** 2).sum(dim=0).mul((n - 1) / n).sqrt()
        if value.numel() == 1:
            return value.item(), err.item()
        return value, err

    def mean(self, name, binsize=1):
        return self.estimate(self.series(name), binsize=binsize)

    def susceptibility(self, binsize=1):
        """V (<m^2> - <|m|>^2)."""
        p = torch.cat([self.series('m2'), self.series('abs_magnetization')], dim=2)
        return self.estimate(p, lambda a: self.volume * (a[..., 0:1] - a[..., 1:2] ** 2), binsize)

    def binder(self, binsize=1):
        """1 - <m^4> / (3 <m^2>^2)."""
        p = torch.cat([self.series('m2'), self.series('m4')], dim=2)
        return self.estimate(p, lambda a: 1 - a[..., 1:2] / (3 * a[..., 0:1] ** 2), binsize)

    def _corr(self, axis, connected):
        p = torch.cat([self.series(self.m.correlator(axis)), self.series('magnetization')], dim=2)
        return p, (lambda a: a[..., :-1] - a[..., -1:] ** 2) if connected else (lambda a: a[..., :-1])

    def correlator(self, axis=None, connected=False, binsize=1):
        """<G_mu(t)>, t = 0 .. L - 1; connected: minus <m>^2."""
        p, fn = self._corr(axis, connected)
        return self.estimate(p, fn, binsize)

    def propagator(self, axis=None, binsize=1):
        """<|sum_t e^{ipt} S_mu(t)|^2> / V at p = 2 pi k / L, k = 0 .. L - 1."""
        return self.estimate(self.series(self.m.propagator(axis)), binsize=binsize)

    def effective_mass(self, axis=None, connected=False, binsize=1):
        """arccosh((G(t - 1) + G(t + 1)) / (2 G(t))) at t = 1 .. L - 2; NaN where the argument is < 1."""
        p, fn = self._corr(axis, connected)

        def mass(a):
            g = fn(a)
            arg = (g[..., :-2] + g[..., 2:]) / (2 * g[..., 1:-1])
            return torch.where(arg >= 1, torch.acosh(arg.clamp(min=1)), torch.full_like(arg, float('nan')))
        return self.estimate(p, mass, binsize)

    def xi2(self, axis=None, binsize=1):
        """The second-moment correlation length sqrt(G~(0) / G~(p_min) - 1) / (2 sin(pi / L)); NaN where the ratio is < 1."""
        L = self.lattice[self.m._axes(axis)[0]]
        p = self.series(self.m.propagator(axis)[:, :2])

        def xi(a):
            r = a[..., 0:1] / a[..., 1:2] - 1
            return torch.where(r >= 0, r.clamp(min=0).sqrt(), torch.full_like(r, float('nan'))) / (2 * math.sin(math.pi / L))
        return self.estimate(p, xi, binsize)

    def tau_int(self, name, c=5.0):
        """(tau, error, W): the integrated autocorrelation time of `name` in steps, tau(W) = 1/2 + sum_{t=1}^{W} rho(t), at
        the Madras-Sokal window, the smallest W with W >= c tau(W); error tau sqrt(2 (2 W + 1) / (steps chains)).  The
        autocovariance is computed per chain by FFT (around the mean of all chains) and averaged over the chains."""
        x = self.series(name)[:, :, 0]
        n, C = x.shape
        x = x - x.mean()
        f = torch.fft.rfft(x, n=2 * n, dim=0)
        acov = torch.fft.irfft(f.real ** 2 + f.imag ** 2, n=2 * n, dim=0)[:n]
        acov = acov.mean(dim=1) / torch.arange(n, 0, -1, dtype=torch.float64, device=x.device)
        rho = acov / acov[0]
        tau = 0.5 + torch.cumsum(rho[1:], dim=0)                    # tau(W) at W = 1 ..
        W = torch.arange(1, n, dtype=torch.float64, device=x.device)
        ok = torch.nonzero(W >= c * tau)
        w = int(ok[0]) if ok.numel() else n - 2
        t = tau[w].item()
        return t, t * math.sqrt(2 * (2 * (w + 1) + 1) / (n * C)), w + 1


# ---------------------------------------------------------------- cluster-improved estimators
IMPROVED_PATHS = (None, 'kernel', 'composed', 'hbm')
SPECTRUM_PATHS = (None, 'hbm')             # of `measure_improved(spectrum_path=...)`: 'hbm' is nf_cluster_spectrum_tiled
MODES_PATHS = (None, 'hbm')                # of `measure_improved(modes_path=...)`: 'hbm' is nf_cluster_modes_tiled


def improved_kernel_applies(cfgs):
    """True where nf_cluster_moments can take the chains: fp32 / fp64 rows on the device, on a lattice of the cluster
    kernel's class (V sizeof <= 64 KiB)."""
    return bool(_on_device(cfgs) and _hip.cluster_moments_supported(tuple(cfgs.shape[1:]), cfgs.dtype))


def route_improved(cfgs):
    """The path that `measure_improved(cfgs, labels)` takes: 'kernel' wherever `improved_kernel_applies`, else
    'composed'.  tools/cluster_bench.py --improved measured nf_cluster_moments 17 to 33 times faster than the composed
    path on an MI355X at 16^2 x 512 and 16^3 x 1024, fp32 and fp64, at kappa = 0.67 and 0.25, far beyond its margin (the
    larger of 10 % and the run's spread; README, "Improved estimators"); the other lattices of the kernel's class were
    not timed and follow by extrapolation."""
    return 'kernel' if improved_kernel_applies(cfgs) else 'composed'


@torch.no_grad()
def measure_improved(cfgs, labels, path=None, momenta=None, spectrum_path=None, workspace=None, modes=None, modes_path=None,
                     modes_workspace=None):
    """(N, *L) configurations and the (N, *L) int32 labels of their cluster decompositions (a Swendsen-Wang sweep's:
    `hmc.cluster(phi)['labels']`, with the field before or after the flip) -> `ImprovedMeasurement`: the averages over
    all 2^Nc assignments of the clusters' signs, in closed form from the clusters' sums M_C (include/normflow_hip.h,
    "cluster-improved estimators").  path=None: what `route_improved` says; 'kernel' (nf_cluster_moments; raises where it
    cannot run), 'composed' (`mcmc.cluster.cluster_moments`: torch ops, any device) or 'hbm' (nf_cluster_moments_tiled:
    the slots in HBM, any lattice on the device; raises on CPU tensors) force one.  `route_improved` never says 'hbm':
    the path is opt-in until the routing is redone from measured classes.
    momenta='all' or an int >= 1: the measurement also carries the spectrum, sum_C |M~_C(2 pi k / L_mu)|^2 at
    k = 1 .. K_mu of every axis (include/normflow_hip.h, "cluster spectrum"), from which `propagator` and `correlator`
    follow where momenta='all'.  path=None / 'kernel' then run nf_cluster_spectrum where `improved_kernel_applies`
    (path=None elsewhere: composed), 'composed' is `mcmc.cluster.cluster_spectrum`, and 'hbm' raises ValueError: there is
    no spectrum on that path key; the tiled spectrum kernel is reached through `spectrum_path`.  `out` is that of the call
    without momenta bit for bit on the same path (its columns are columns of the spectrum's row).
    spectrum_path='hbm' (opt-in; needs momenta, and path None or 'hbm'; ValueError otherwise): nf_cluster_spectrum_tiled,
    the slots in HBM, any lattice on the device (raises on CPU tensors); `out` is then that of path='hbm' bit for bit.
    `workspace`: a uint8 tensor for that kernel (`_hip.cluster_spectrum_tiled`), None: one per call; ValueError where it
    is given without spectrum_path.  Without
    spectrum_path every call does what it did: path=None beyond one CU stays on the composed path.
    modes=[(n0, ..), ...]: P <= 512 integer momentum vectors with one component per axis, on or off the axes, negative
    components allowed (include/normflow_hip.h, "cluster modes"): the measurement also carries `.modes`, the vectors
    reduced to 0 .. L_mu - 1, and `.mode_power` (N, P) = sum_C |M~_C(p)|^2 at p_mu = 2 pi n_mu / L_mu, from which
    `mode_propagator` and `mode_correlator` follow.  It runs on its own: path=None / 'kernel' take nf_cluster_modes where
    `improved_kernel_applies` (path=None elsewhere: composed), 'composed' is `mcmc.cluster.cluster_modes`, and 'hbm'
    raises ValueError unless `modes_path` is given: the tiled modes kernel is reached through that keyword, as the tiled
    spectrum through `spectrum_path`.  `momenta` keeps its meaning beside it; everything else of the measurement, `out`
    included, is that of the call without `modes` bit for bit.
    modes_path='hbm' (opt-in; needs modes, and path None or 'hbm'; ValueError otherwise): `.modes` and `.mode_power` are
    nf_cluster_modes_tiled's, the slots in HBM, any lattice on the device whose lcm of extents is at most 65536 (raises
    NormflowHipError on CPU tensors).  `modes_workspace`: a uint8 tensor for that kernel (`_hip.cluster_modes_tiled`),
    None: one per call; ValueError where it is given without modes_path.  Without modes_path every call does what it
    did: path=None beyond one CU stays on the composed path."""
    if path not in IMPROVED_PATHS:
        raise ValueError(f"path must be None, 'kernel', 'composed' or 'hbm', got {path!r}")
    if not 1 <= cfgs.ndim - 1 <= 4:
        raise ValueError(f"measure_improved: configurations (N, *L) with 1 to 4 lattice axes, got {tuple(cfgs.shape)}")
    lat = tuple(cfgs.shape[1:])
    if spectrum_path not in SPECTRUM_PATHS:
        raise ValueError(f"spectrum_path must be None or 'hbm', got {spectrum_path!r}")
    if workspace is not None and spectrum_path is None:
        raise ValueError("measure_improved: workspace is the workspace of spectrum_path='hbm' (nf_cluster_spectrum_tiled); "
                         "no other path takes one")
    if spectrum_path is not None:
        if momenta is None:
            raise ValueError("measure_improved: spectrum_path='hbm' is the path of the spectrum: it needs momenta")
        if path not in (None, 'hbm'):
            raise ValueError(f"measure_improved: spectrum_path='hbm' goes with path None or 'hbm', got path={path!r}")
    if modes_path not in MODES_PATHS:
        raise ValueError(f"modes_path must be None or 'hbm', got {modes_path!r}")
    if modes_workspace is not None and modes_path is None:
        raise ValueError("measure_improved: modes_workspace is the workspace of modes_path='hbm' (nf_cluster_modes_tiled); "
                         "no other path takes one")
    if modes_path is not None:
        if modes is None:
            raise ValueError("measure_improved: modes_path='hbm' is the path of the modes: it needs modes")
        if path not in (None, 'hbm'):
            raise ValueError(f"measure_improved: modes_path='hbm' goes with path None or 'hbm', got path={path!r}")
    if modes is not None:
        if path == 'hbm' and modes_path is None:
            raise ValueError("measure_improved: no modes on path 'hbm' (nf_cluster_moments_tiled has no modes form): use "
                             "modes_path='hbm' (nf_cluster_modes_tiled), or path='composed', for lattices beyond one CU")
        try:
            _hip.modes_list(lat, modes)
        except _hip.NormflowHipError as e:
            raise ValueError(f"measure_improved: {e}") from None
    if modes_path == 'hbm':
        _hip._require_device(cfgs, labels)
    im = _measure_improved(cfgs, labels, path, momenta, spectrum_path, workspace, lat)
    if modes_path == 'hbm':
        r = _hip.cluster_modes_tiled(cfgs.contiguous(), labels.contiguous(), modes, workspace=modes_workspace)
        im.modes, im.mode_power = r['modes'], r['out'][:, 2:]
    elif modes is not None:
        if path is None:
            path = 'kernel' if improved_kernel_applies(cfgs) else 'composed'
        if path == 'kernel':
            r = _hip.cluster_modes(cfgs.contiguous(), labels.contiguous(), modes)
        else:
            from ..mcmc.cluster import cluster_modes
            r = cluster_modes(cfgs, labels, modes)
        im.modes, im.mode_power = r['modes'], r['out'][:, 2:]
    return im


def _measure_improved(cfgs, labels, path, momenta, spectrum_path, workspace, lat):
    """`measure_improved` without `modes`, its arguments checked."""
    if momenta is not None:
        if path == 'hbm' and spectrum_path is None:
            raise ValueError("measure_improved: no spectrum on path 'hbm' (nf_cluster_moments_tiled has no spectrum form): "
                             "use spectrum_path='hbm' (nf_cluster_spectrum_tiled), or path='composed', for lattices beyond "
                             "one CU")
        if momenta != 'all' and (isinstance(momenta, bool) or not isinstance(momenta, int) or momenta < 1):
            raise ValueError(f"momenta must be None, 'all' or an int >= 1, got {momenta!r}")
        if spectrum_path == 'hbm':
            r = _hip.cluster_spectrum_tiled(cfgs.contiguous(), labels.contiguous(), momenta, workspace=workspace)
            return ImprovedMeasurement.from_spectrum(r['out'], r['status'], lat, r['momenta'])
        if path is None:
            path = 'kernel' if improved_kernel_applies(cfgs) else 'composed'
        if path == 'kernel':
            r = _hip.cluster_spectrum(cfgs.contiguous(), labels.contiguous(), momenta)
        else:
            from ..mcmc.cluster import cluster_spectrum
            r = cluster_spectrum(cfgs, labels, momenta)
        return ImprovedMeasurement.from_spectrum(r['out'], r['status'], lat, r['momenta'])
    if path is None:
        path = route_improved(cfgs)
    if path == 'kernel':
        r = _hip.cluster_moments(cfgs.contiguous(), labels.contiguous())
    elif path == 'hbm':
        r = _hip.cluster_moments_tiled(cfgs.contiguous(), labels.contiguous())
    else:
        from ..mcmc.cluster import cluster_moments
        r = cluster_moments(cfgs, labels)
    return ImprovedMeasurement(r['out'], r['status'], lat)


class ImprovedMeasurement:
    """Per-row sign-averaged sums of N configurations, float64: sum_m2 = sum_C M_C^2, sum_m4c = sum_C M_C^4, prop1 (N, d) =
    sum_C |sum_{x in C} phi(x) e^{i p x_mu}|^2 at p = 2 pi / L_mu per axis (an axis of extent 1 repeats sum_m2); status (N)
    int32, 1 = a refused row (all NaN); lattice, volume.  With the clusters' signs averaged,
        <(sum phi)^2> = sum M_C^2,   <(sum phi)^4> = 3 (sum M_C^2)^2 - 2 sum M_C^4,   <|phi~(p)|^2> = sum_C |M~_C(p)|^2,
    and all three are invariant under the flips: the field before or after the sweep gives the same bits.
    `spectrum` (None, or a list of d tensors (N, K_mu)): the last of the three at p = 2 pi k / L_mu, k = 1 .. K_mu, and
    `momenta` the K_mu; `propagator` and `correlator` need the full spectrum, K_mu = L_mu // 2 (momenta='all').
    `modes` (None, or a tuple of P momentum vectors reduced to 0 .. L_mu - 1) and `mode_power` (N, P): the same sum at
    p_mu = 2 pi n_mu / L_mu of every listed vector (`measure_improved(..., modes=...)`)."""

    def __init__(self, out, status, lattice, spectrum=None, momenta=None, modes=None, mode_power=None):
        self.out = out                        # (N, 2 + d): the three below side by side
        self.sum_m2, self.sum_m4c, self.prop1, self.status = out[:, 0], out[:, 1], out[:, 2:], status
        self.lattice = tuple(lattice)
        self.volume = math.prod(self.lattice)
        self.spectrum = None if spectrum is None else list(spectrum)
        if self.spectrum is not None:
            momenta = tuple(int(t.shape[1]) for t in self.spectrum) if momenta is None else tuple(int(k) for k in momenta)
            if len(self.spectrum) != len(self.lattice) or momenta != tuple(int(t.shape[1]) for t in self.spectrum):
                raise ValueError(f"spectrum: one (N, K_mu) tensor per axis of {self.lattice} with K = {momenta}")
        self.momenta = momenta if self.spectrum is not None else None
        self.modes = None if modes is None else tuple(tuple(int(n) for n in m) for m in modes)
        self.mode_power = mode_power if self.modes is not None else None
        if self.modes is not None and (mode_power is None or tuple(mode_power.shape) != (out.shape[0], len(self.modes))):
            raise ValueError(f"mode_power: one (N, P) tensor for the P = {len(self.modes)} momenta")

    @classmethod
    def from_spectrum(cls, row, status, lattice, momenta):
        """From the (N, 2 + sum K_mu) rows of the cluster spectrum: `out` takes columns 0 and 1 and the k = 1 column of
        every axis (column 0 for an axis of extent 1), which are `cluster_moments`' bits."""
        at, parts, cols = 2, [], [0, 1]
        for K in momenta:
            parts.append(row[:, at:at + K])
            cols.append(at if K else 0)
            at += K
        return cls(torch.stack([row[:, c] for c in cols], dim=1), status, lattice, parts, momenta)    # slices: no index tensor

    def __len__(self):
        return self.sum_m2.shape[0]

    _axes = Measurement._axes

    @classmethod
    def cat(cls, parts, lattice, device, momenta=None, modes=None):
        """The rows of `parts` (ImprovedMeasurements of one lattice) one after the other; none: an empty one on `device`
        (with the empty spectrum of `momenta`, the K_mu, and the empty mode_power of `modes`, where given)."""
        if not parts:
            spec = None if momenta is None else [torch.empty((0, K), dtype=torch.float64, device=device) for K in momenta]
            power = None if modes is None else torch.empty((0, len(modes)), dtype=torch.float64, device=device)
            return cls(torch.empty((0, 2 + len(lattice)), dtype=torch.float64, device=device),
                       torch.empty((0,), dtype=torch.int32, device=device), lattice, spec, momenta, modes, power)
        spec = None
        if parts[0].spectrum is not None:
            spec = [torch.cat([p.spectrum[mu] for p in parts]) for mu in range(len(lattice))]
        power = None if parts[0].modes is None else torch.cat([p.mode_power for p in parts])
        return cls(torch.cat([p.out for p in parts]), torch.cat([p.status for p in parts]), lattice, spec, parts[0].momenta,
                   parts[0].modes, power)

    def rows(self, col):
        """The same rows laid out by `col`: row i goes to row col[i] (the ladder's rung order)."""
        spec = None if self.spectrum is None else [torch.empty_like(t).index_copy_(0, col, t) for t in self.spectrum]
        power = None if self.modes is None else torch.empty_like(self.mode_power).index_copy_(0, col, self.mode_power)
        return type(self)(torch.empty_like(self.out).index_copy_(0, col, self.out),
                          torch.empty_like(self.status).index_copy_(0, col, self.status), self.lattice, spec, self.momenta,
                          self.modes, power)

    def pick(self, fn):
        """The measurement of the rows that `fn` picks from every (N, ...) tensor (the ladder's rows of one rung)."""
        spec = None if self.spectrum is None else [fn(t) for t in self.spectrum]
        power = None if self.modes is None else fn(self.mode_power)
        return type(self)(fn(self.out), fn(self.status), self.lattice, spec, self.momenta, self.modes, power)

    def m2(self):
        """<m^2>_signs = sum M_C^2 / V^2."""
        return self.sum_m2 / self.volume ** 2

    def m4(self):
        """<m^4>_signs = (3 (sum M_C^2)^2 - 2 sum M_C^4) / V^4."""
        return (3 * self.sum_m2 ** 2 - 2 * self.sum_m4c) / self.volume ** 4

    def propagator0(self):
        """The improved `Measurement.propagator` column 0: sum M_C^2 / V."""
        return self.sum_m2 / self.volume

    def propagator1(self, axis=None):
        """The improved `Measurement.propagator` column 1, sum_C |M~_C(p_min)|^2 / V; axis=None: the mean over the axes
        (of equal extents, as in `Measurement`)."""
        axes = self._axes(axis)
        return self.prop1[:, axes].sum(dim=1) / (len(axes) * self.volume)

    def has_spectrum(self):
        """True where the measurement carries the spectrum at all momenta, K_mu = L_mu // 2 of every axis."""
        return self.spectrum is not None and all(K == (n // 2 if n > 1 else 0) for K, n in zip(self.momenta, self.lattice))

    def _power(self, mu):
        """(N, L) P_mu(k) = sum_C |M~_C(2 pi k / L)|^2, k = 0 .. L - 1: P(0) = sum M_C^2 and P(L - k) = P(k)."""
        if not self.has_spectrum():
            raise ValueError("the propagator and the correlator need the spectrum at all momenta: measure with momenta='all'"
                             + ("" if self.spectrum is None else f" (this one has K = {self.momenta} on {self.lattice})"))
        L, half = self.lattice[mu], self.spectrum[mu]
        k = torch.arange(L, device=half.device)
        fold = torch.minimum(k, L - k)                              # 0 .. L // 2
        return torch.cat([self.sum_m2.unsqueeze(1), half], dim=1)[:, fold]

    def propagator(self, axis=None):
        """(N, L) the improved `Measurement.propagator`: P_mu(k) / V at p = 2 pi k / L, k = 0 .. L - 1."""
        axes = self._axes(axis)
        return sum(self._power(mu) for mu in axes) / (len(axes) * self.volume)

    def correlator(self, axis=None):
        """(N, L) the improved `Measurement.correlator`: G_mu(t) = (1 / V^2) sum_k P_mu(k) cos(2 pi k t / L) in float64;
        axis=None: the mean over the axes."""
        axes = self._axes(axis)
        out = 0
        for mu in axes:
            P = self._power(mu)
            L = self.lattice[mu]
            k = torch.arange(L, dtype=torch.float64, device=P.device)
            cos = torch.cos(2.0 * math.pi * ((k[:, None] * k[None, :]) % L) / L)
            out = out + P @ cos / self.volume ** 2
        return out / len(axes)


    def _modes(self, what):
        if self.modes is None:
            raise ValueError(f"{what} needs the modes: measure with modes=[(n0, ...), ...]")

    def mode_propagator(self):
        """(N, P) sum_C |M~_C(p)|^2 / V at the momenta of `modes`, in list order: the improved |phi~(p)|^2 / V."""
        self._modes('mode_propagator')
        return self.mode_power / self.volume

    def mode_correlator(self, axis, spatial):
        """(N, L) the improved time-slice correlator along `axis` at the spatial momentum `spatial` (the components of the
        other axes, in their order): G(t; p) = (1 / V^2) sum_{k=0}^{L-1} P(k, p) cos(2 pi k t / L) in float64, in
        `correlator`'s normalisation.  It needs all L momenta of `correlator_modes(lattice, axis, spatial)` among `modes`
        and raises a ValueError that names the missing ones otherwise."""
        self._modes('mode_correlator')
        want = correlator_modes(self.lattice, axis, spatial)
        have = {m: i for i, m in reversed(list(enumerate(self.modes)))}          # the first place of a repeated momentum
        missing = [m for m in want if m not in have]
        if missing:
            raise ValueError(f"mode_correlator(axis={axis}, spatial={tuple(spatial)}) needs all {len(want)} momenta along "
                             f"the axis; missing from modes: {missing}")
        L = len(want)
        P = torch.stack([self.mode_power[:, have[m]] for m in want], dim=1)
        k = torch.arange(L, dtype=torch.float64, device=P.device)
        cos = torch.cos(2.0 * math.pi * ((k[:, None] * k[None, :]) % L) / L)
        return P @ cos / self.volume ** 2


def correlator_modes(lattice, axis, spatial):
    """The L momenta (k, p) that `mode_correlator(axis, spatial)` needs, k = 0 .. L - 1 along `axis` of `lattice` and
    the components `spatial` (one per other axis, in their order) elsewhere, reduced to 0 .. L_mu - 1."""
    lattice = tuple(int(n) for n in lattice)
    axis = range(len(lattice))[axis]
    spatial = tuple(spatial)
    if len(spatial) != len(lattice) - 1 or any(isinstance(n, bool) or not isinstance(n, int) for n in spatial):
        raise ValueError(f"spatial: {len(lattice) - 1} integer components, those of the axes of {lattice} other than {axis}, "
                         f"got {spatial!r}")
    return [tuple(n % L for n, L in zip(spatial[:axis] + (k,) + spatial[axis:], lattice)) for k in range(lattice[axis])]


@torch.no_grad()
def measure_modes(cfgs, modes, labels=None, path=None, modes_path=None):
    """`measure_improved(cfgs, labels, path=path, modes=modes)`: the `ImprovedMeasurement` with `.modes` and `.mode_power`.
    labels=None is the decomposition into ONE cluster (all labels 0): with it `mode_power` is the plain |phi~(p)|^2 of
    every row, in the estimators' fixed point and from the same kernel, at momenta that `Measurement.propagator` does not
    reach.  path=None | 'kernel' | 'composed': None takes nf_cluster_modes where `improved_kernel_applies`, else the
    composed path.  modes_path='hbm' (opt-in, with path None or 'hbm'): nf_cluster_modes_tiled, any lattice on the device."""
    if modes_path not in MODES_PATHS:
        raise ValueError(f"modes_path must be None or 'hbm', got {modes_path!r}")
    if path not in ((None, 'kernel', 'composed') if modes_path is None else (None, 'hbm')):
        raise ValueError(f"path must be None, 'kernel' or 'composed' (with modes_path='hbm': None or 'hbm'), got {path!r}")
    if labels is None:
        labels = torch.zeros(cfgs.shape, dtype=torch.int32, device=cfgs.device)
    if modes_path is None:
        return measure_improved(cfgs, labels, path=path, modes=modes)
    return measure_improved(cfgs, labels, path=path, modes=modes, modes_path=modes_path)


class ImprovedEnsemble(Ensemble):
    """`Ensemble` for an `ImprovedMeasurement` of sampler rows (sweeps, n_chains), the first `drop` sweeps left out: the
    same jackknife (`estimate`) and `tau_int`, on the improved series 'm2' and 'm4'."""

    NAMES = ('m2', 'm4')

    def series(self, name):
        if torch.is_tensor(name):
            t = name
        elif name not in self.NAMES:
            raise ValueError(f"unknown improved observable {name!r}: one of {self.NAMES}")
        else:
            t = self.m.m2() if name == 'm2' else self.m.m4()
        t = t.detach().double().cpu()
        return t.reshape(self.steps + self.drop, self.n_chains, -1)[self.drop:]

    def susceptibility(self, binsize=1):
        """V <m^2>: the SYMMETRIC definition.  There is no improved <|m|> (|m| is not a polynomial in the signs), so this
        is not `Ensemble.susceptibility`'s V (<m^2> - <|m|>^2); the two agree where <|m|> vanishes."""
        return self.estimate(self.series('m2'), lambda a: self.volume * a, binsize)

    def binder(self, binsize=1):
        """1 - <m^4> / (3 <m^2>^2), both moments improved."""
        return Ensemble.binder(self, binsize)

    def propagator1(self, axis=None, binsize=1):
        """<sum_C |M~_C(p_min)|^2> / V."""
        return self.estimate(self.series(self.m.propagator1(axis)), binsize=binsize)

    def xi2(self, axis=None, binsize=1):
        """`Ensemble.xi2`'s formula on the improved propagator at p = 0 and p_min."""
        L = self.lattice[self.m._axes(axis)[0]]
        p = self.series(torch.stack([self.m.propagator0(), self.m.propagator1(axis)], dim=1))

        def xi(a):
            r = a[..., 0:1] / a[..., 1:2] - 1
            return torch.where(r >= 0, r.clamp(min=0).sqrt(), torch.full_like(r, float('nan'))) / (2 * math.sin(math.pi / L))
        return self.estimate(p, xi, binsize)

    def _spectral(self, what):
        if self.m.spectrum is None:
            raise NotImplementedError(f"an ImprovedEnsemble has {what} only on a measurement with a spectrum (measure with "
                                      "momenta='all'); without one it has m2, m4, susceptibility, binder, propagator1, xi2 "
                                      "and tau_int")

    def _corr(self, axis, connected):
        self._spectral('a correlator')
        if connected:
            raise ValueError("connected=True: the sign-averaged <m> is 0, the improved correlator is its own connected part")
        return self.series(self.m.correlator(axis)), (lambda a: a)

    def correlator(self, axis=None, connected=False, binsize=1):
        """<G_mu(t)> improved, t = 0 .. L - 1 (`ImprovedMeasurement.correlator`); connected=True raises ValueError."""
        p, fn = self._corr(axis, connected)
        return self.estimate(p, fn, binsize)

    def propagator(self, axis=None, binsize=1):
        """<sum_C |M~_C(p)|^2> / V at p = 2 pi k / L, k = 0 .. L - 1."""
        self._spectral('a propagator')
        return self.estimate(self.series(self.m.propagator(axis)), binsize=binsize)

    def effective_mass(self, axis=None, connected=False, binsize=1):
        """`Ensemble.effective_mass`'s formula on the improved correlator."""
        self._spectral('an effective mass')
        return Ensemble.effective_mass(self, axis, connected, binsize)

    def mode_propagator(self, binsize=1):
        """<sum_C |M~_C(p)|^2> / V at the momenta of the measurement's `modes`, in list order."""
        return self.estimate(self.series(self.m.mode_propagator()), binsize=binsize)

    def mode_correlator(self, axis, spatial, binsize=1):
        """<G(t; p)> improved, t = 0 .. L - 1 (`ImprovedMeasurement.mode_correlator`)."""
        return self.estimate(self.series(self.m.mode_correlator(axis, spatial)), binsize=binsize)

    def mode_effective_mass(self, axis, spatial, binsize=1):
        """`Ensemble.effective_mass`'s formula on `mode_correlator(axis, spatial)`: the energy E(p) of the state at the
        spatial momentum, arccosh((G(t - 1) + G(t + 1)) / (2 G(t))) at t = 1 .. L - 2; NaN where the argument is < 1."""
        def mass(g):
            arg = (g[..., :-2] + g[..., 2:]) / (2 * g[..., 1:-1])
            return torch.where(arg >= 1, torch.acosh(arg.clamp(min=1)), torch.full_like(arg, float('nan')))
        return self.estimate(self.series(self.m.mode_correlator(axis, spatial)), mass, binsize)
