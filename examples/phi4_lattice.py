#!/usr/bin/env python3
"""Train a phi^4 flow on an MI355X with this package -- the network of the reference's
examples/scalar_affine.py (spectral block, DistConvertor_, affine couplings with ConvAct nets,
DistConvertor_), or a stack of RQ-spline couplings, assembled from the same names.

    python examples/phi4_lattice.py --lat 8,8 --epochs 500
    python examples/phi4_lattice.py --lat 16,16,16 --kind rqs --layers 4 --epochs 100
    torchrun-free data parallel:  --nranks 8   (device_handler.spawnprocesses, one process per GPU)
    python examples/phi4_lattice.py --lat 8,8 --ladder    no fit: a ladder of kappas across the transition sampled by
                                                           model.hmc.ladder, chi, U4 and tau_int(m) per rung, without and
                                                           with replica exchange
    python examples/phi4_lattice.py --lat 8,8 --ladder --cluster    the same, and once more with a cluster sweep of every
                                                           chain at its rung's coupling before every step
    python examples/phi4_lattice.py --lat 16,16 --hmc     after the fit: <phi^2> from model.mcmc next to model.hmc, then
                                                          chi, the Binder cumulant, xi_2 and tau_int(m) of both
    python examples/phi4_lattice.py --lat 16,16 --hmc --integrator omelyan    the same with model.hmc on the second-order
                                                           minimum-norm integrator (or omf4) instead of leapfrog
    python examples/phi4_lattice.py --lat 16,16 --hmc --fourier 0.25    the same, and model.hmc once more with the Fourier-
                                                           accelerated kinetic term: acceptance, <phi^2>, chi, tau_int both ways
    python examples/phi4_lattice.py --lat 8,8 --hmc --cluster    the same, and model.hmc once more with a cluster sweep of
                                                          the signs before every step: tau_int(m) with and without sweeps
    python examples/phi4_lattice.py --lat 8,8 --hmc --cluster --improved    the same, and chi = V <m^2>, U4 and xi_2 of that
                                                          run both ways: from the one sign assignment the sweeps left, and
                                                          averaged over all of them (the cluster-improved estimators)
    python examples/phi4_lattice.py --lat 8,8 --hmc --cluster --improved --correlator    that, and G(t) and m_eff(t) both ways
    python examples/phi4_lattice.py --lat 8,8 --hmc --cluster --improved --modes         that, and G(p) off the axes and m_eff of G(t; p = (1, 0, ...))
"""
import argparse
import math
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # run from a source checkout

import normflow__amd as nf          # the reference:  import normflow as nf
from normflow__amd.action import ScalarPhi4Action
from normflow__amd.lib import Ensemble, fmt_val_err
from normflow__amd.lib.observables import ImprovedEnsemble, correlator_modes, measure_modes
from normflow__amd.mask import EvenOddMask
from normflow__amd.nn import (AffineCoupling_, ConvAct, DistConvertor_, FFTNet_, MeanFieldNet_, ModuleList_,
                              PSDBlock_, RQSplineCoupling_)
from normflow__amd.prior import NormalPrior


def build_net(lat, kind, layers, knots, transform='fft'):
    d = len(lat)
    mask = EvenOddMask(shape=lat)

    def param_net(channels):
        return ConvAct(in_channels=1, out_channels=channels, hidden_sizes=[8, 8], kernel_size=3, conv_dim=d,
                       acts=('tanh', 'tanh', None), bias=(kind == 'rqs'))

    if kind == 'affine':
        return ModuleList_([
            PSDBlock_(mfnet_=MeanFieldNet_.build(knots_len=10, symmetric=True, final_scale=True, smooth=True),
                      fftnet_=FFTNet_.build(lat, knots_len=10, ignore_zeromode=True, transform=transform)),
            DistConvertor_(50, symmetric=True, smooth=True),
            AffineCoupling_([param_net(2) for _ in range(layers)], mask=mask),
            DistConvertor_(50, symmetric=True, smooth=True)])
    return ModuleList_([
        RQSplineCoupling_([param_net(3 * knots - 2) for _ in range(layers)], mask=mask, xlim=(-5, 5), ylim=(-5, 5),
                          extrap={'left': 'linear', 'right': 'linear'})])


def fit(model, **kw):
    model.fit(**kw)


def phi2(y, n_chains, drop):
    """(mean, standard error across chains) of <phi^2> from sampler rows (row r = step r // C of chain r % C)."""
    y = y.double().reshape(y.shape[0] // n_chains, n_chains, -1)[drop:]
    per_chain = (y ** 2).mean(dim=(0, 2))
    return per_chain.mean().item(), per_chain.std().item() / n_chains ** 0.5


def observables(model, y, n_chains, drop):
    """chi, the Binder cumulant, xi_2 (mean over the axes of a cubic lattice, else along axis 0) and tau_int(m) of sampler
    rows, through model.measure (one pass over the rows on the device) and Ensemble (errors: jackknife over the chains)."""
    e = Ensemble(model.measure(y), n_chains=n_chains, drop=drop)
    axis = None if len(set(e.lattice)) == 1 else 0
    tau, tau_err, window = e.tau_int('magnetization')
    return "chi %s   U4 %s   xi_2 %s   tau_int(m) %s (W = %d)" % (
        fmt_val_err(*e.susceptibility()), fmt_val_err(*e.binder()), fmt_val_err(*e.xi2(axis)), fmt_val_err(tau, tau_err), window)


def tau_ints(model, y, n_chains, drop):
    """tau_int of the magnetization and of phi^2 of sampler rows, with their errors."""
    e = Ensemble(model.measure(y), n_chains=n_chains, drop=drop)
    return ", ".join(fmt_val_err(*e.tau_int(name)[:2]) for name in ('magnetization', 'phi2'))


def both_ways(m, n_chains, drop):
    """chi = V <m^2> (the symmetric definition: there is no improved <|m|>), U4 and xi_2 of a measurement that carries
    `.improved`, from the sign assignment the sweeps left and averaged over all sign assignments, with their errors."""
    e, ie = Ensemble(m, n_chains=n_chains, drop=drop), ImprovedEnsemble(m.improved, n_chains=n_chains, drop=drop)
    axis = None if len(set(e.lattice)) == 1 else 0
    chi, chi_err = e.mean('m2')
    lines = ["            chi = V<m^2> %s   U4 %s   xi_2 %s" % (
        fmt_val_err(e.volume * chi, e.volume * chi_err), fmt_val_err(*e.binder()), fmt_val_err(*e.xi2(axis))),
             "  improved  chi = V<m^2> %s   U4 %s   xi_2 %s" % (
        fmt_val_err(*ie.susceptibility()), fmt_val_err(*ie.binder()), fmt_val_err(*ie.xi2(axis)))]
    return "\n".join(lines)


def correlators(m, n_chains, drop):
    """G(t) and m_eff(t) along axis 0 of a measurement whose `.improved` carries the full spectrum (momenta='all'): from
    the sign assignment the sweeps left and averaged over all sign assignments, with their errors."""
    e, ie = Ensemble(m, n_chains=n_chains, drop=drop), ImprovedEnsemble(m.improved, n_chains=n_chains, drop=drop)
    (g, ge), (ig, ige) = e.correlator(axis=0), ie.correlator(axis=0)
    (ms, mse), (ims, imse) = e.effective_mass(axis=0), ie.effective_mass(axis=0)
    lines = ["   t   G(t)                    improved G(t)           m_eff(t)                improved m_eff(t)"]
    for t in range(len(g) // 2 + 1):
        mass = ("%-23s %s" % (fmt_val_err(ms[t - 1].item(), mse[t - 1].item()), fmt_val_err(ims[t - 1].item(), imse[t - 1].item()))
                if 1 <= t <= len(ms) else "")
        lines.append("  %2d   %-23s %-23s %s" % (t, fmt_val_err(g[t].item(), ge[t].item()), fmt_val_err(ig[t].item(), ige[t].item()),
                                                 mass))
    return "\n".join(lines)


def example_modes(lat):
    """(off-axis momenta, the spatial momentum (1, 0, ...), the L momenta of its correlator along axis 0)."""
    d = len(lat)
    off = [n for n in ((1, 1) + (0,) * (d - 2), (1, 2) + (0,) * (d - 2), (2, -1) + (0,) * (d - 2), (2, 2) + (0,) * (d - 2),
                       (1,) * d) if d >= 2]
    spatial = ((1,) + (0,) * (d - 2)) if d >= 2 else ()
    return list(dict.fromkeys(off)), spatial, correlator_modes(lat, 0, spatial)


def off_axis(m, y, lat, n_chains, drop):
    """G(p) = <|phi~(p)|^2> / V against phat^2 = sum_mu 4 sin^2(pi n_mu / L_mu) at a few off-axis momenta, and m_eff of the
    time-slice correlator at the spatial momentum (1, 0, ...): cluster-improved (`m.improved`, measured with modes) next to
    plain (`measure_modes` of the rows `y` with one cluster: the same kernel, the same fixed point)."""
    off, spatial, _ = example_modes(lat)
    ie = ImprovedEnsemble(m.improved, n_chains=n_chains, drop=drop)
    pe = ImprovedEnsemble(measure_modes(y, m.improved.modes), n_chains=n_chains, drop=drop)
    (ig, ige), (pg, pge) = ie.mode_propagator(), pe.mode_propagator()
    lines = ["   n             phat^2    G(p)                    improved G(p)"]
    for i, n in enumerate(off):
        phat2 = sum(4 * math.sin(math.pi * k / L) ** 2 for k, L in zip(n, lat))
        lines.append("   %-12s  %7.4f   %-23s %s" % (n, phat2, fmt_val_err(pg[i].item(), pge[i].item()), fmt_val_err(ig[i].item(), ige[i].item())))
    (ims, imse), (pms, pmse) = ie.mode_effective_mass(0, spatial), pe.mode_effective_mass(0, spatial)
    lines.append("   t   m_eff(t) of G(t; p = %s)   improved" % (spatial,))
    for t in range(1, lat[0] // 2 + 1):
        if t <= len(ims):
            lines.append("  %2d   %-23s %s" % (t, fmt_val_err(pms[t - 1].item(), pmse[t - 1].item()), fmt_val_err(ims[t - 1].item(), imse[t - 1].item())))
    return "\n".join(lines)


# trajectories of length 1 at about the same cost in force evaluations: n_md of each integrator, dt = 1 / n_md
INTEGRATOR_N_MD = dict(leapfrog=10, omelyan=5, omf4=2)


def compare_with_hmc(model, n_chains=64, rows=128, cluster=False, improved=False, integrator='leapfrog', correlator=False,
                     spectrum_path=None, fourier=None, fourier_path=None, modes=False, modes_path=None):
    """<phi^2> of the trained flow + Metropolis next to hybrid Monte Carlo on the action itself (exact up to its own
    statistical error; the first quarter of every chain is dropped as thermalisation), then the observables of both.
    `cluster`: also model.hmc with a Swendsen-Wang sweep of the signs before every recorded step (cluster_every=1), so
    that tau_int(m) stands next to the one without sweeps.  `integrator`: model.hmc's integration scheme, at 10 force
    evaluations per trajectory of length 1 whichever it is.  `fourier`: model.hmc once more with fa_mass_sq, by
    `fourier_path` (None: the sampler's choice; 'fa', 'composed', or 'fa_tiled', the opt-in kernel for chains in HBM)."""
    n_md = INTEGRATOR_N_MD[integrator]
    hmc = dict(n_chains=n_chains, n_md=n_md, dt=1.0 / n_md, integrator=integrator)
    y = model.mcmc.sample(n_chains * rows, n_chains=n_chains)
    print("<phi^2>  model.mcmc  %.5f +- %.5f   (accept rate %.3f)" % (*phi2(y, n_chains, rows // 4), model.mcmc.history.accept_rate[-1]))
    obs = observables(model, y, n_chains, rows // 4)
    y = model.hmc.sample(n_chains * rows, **hmc)
    print("<phi^2>  model.hmc   %.5f +- %.5f   (%s, n_md = %d: accept rate %.3f, rms dH %.3g)"
          % (*phi2(y, n_chains, rows // 4), integrator, n_md, model.hmc.history.accept_rate[-1], model.hmc.history.dh_rms[-1]))
    print("model.mcmc  " + obs)
    print("model.hmc   " + observables(model, y, n_chains, rows // 4))
    if fourier is not None:
        plain_tau = tau_ints(model, y, n_chains, rows // 4)
        model.hmc.start(n_chains=n_chains)
        y = model.hmc.sample(n_chains * rows, fa_mass_sq=fourier, path=fourier_path, **hmc)
        print("<phi^2>  model.hmc, fa_mass_sq=%g   %.5f +- %.5f   (accept rate %.3f, rms dH %.3g)"
              % (fourier, *phi2(y, n_chains, rows // 4), model.hmc.history.accept_rate[-1], model.hmc.history.dh_rms[-1]))
        print("model.hmc, fa_mass_sq=%g   " % fourier + observables(model, y, n_chains, rows // 4))
        print("tau_int(m), tau_int(phi^2):   plain %s   accelerated %s" % (plain_tau, tau_ints(model, y, n_chains, rows // 4)))
    if cluster:
        model.hmc.start(n_chains=n_chains)
        y = model.hmc.sample(n_chains * rows, cluster_every=1, **hmc)
        big = model.hmc.last['cluster'][..., 2].double().mean().item() / model.prior.nvar
        print("<phi^2>  model.hmc, cluster_every=1   %.5f +- %.5f   (accept rate %.3f, mean largest cluster %.2f of the lattice)"
              % (*phi2(y, n_chains, rows // 4), model.hmc.history.accept_rate[-1], big))
        print("model.hmc, cluster_every=1   " + observables(model, y, n_chains, rows // 4))
        if improved:
            lat = tuple(model.prior.shape)
            lst = (lambda off, spatial, along: off + along)(*example_modes(lat)) if modes and len(lat) >= 2 else None
            m = model.hmc.measure(n_chains * rows, cluster_every=1, improved=True, momenta='all' if correlator else None,
                                  spectrum_path=spectrum_path if correlator else None, modes=lst, return_rows=lst is not None,
                                  **({} if lst is None or modes_path is None else dict(modes_path=modes_path)), **hmc)
            if lst is not None:
                m, y = m
            print("model.hmc, cluster_every=1, the next %d steps both ways (sweeps and steps coincide: drop = 0)" % rows)
            print(both_ways(m, n_chains, 0))
            if correlator:
                print(correlators(m, n_chains, 0))
            if lst is not None:
                print(off_axis(m, y, lat, n_chains, 0))


def ladder_scan(lat, m_sq, lambd, kappas, replicas=32, steps=600, cluster=False):
    """A coupling ladder across the transition in ONE launch per step: chi, the Binder cumulant and tau_int(m) per rung
    from model.hmc.ladder(...).measure (nothing stored), without and with replica exchange between neighbouring rungs.
    `cluster`: a third run with exchanges and a Swendsen-Wang sweep of every chain, at the hopping coefficient of the rung
    it holds, before every step (cluster_every=1).  The first quarter of every run is dropped as thermalisation."""
    from normflow__amd.action import ScalarPhi4Ladder
    ladder = ScalarPhi4Ladder(kappa=kappas, m_sq=m_sq, lambd=lambd)
    model = nf.Model(net_=None, prior=NormalPrior(shape=lat), action=ladder.rung(0))
    K, C = len(ladder), len(ladder) * replicas
    for every, sweeps in ((0, 0), (1, 0)) + (((1, 1),) if cluster else ()):
        sampler = model.hmc.ladder(ladder)
        ms = sampler.measure(steps * C, n_chains=C, n_md=10, dt=0.1, exchange_every=every, cluster_every=sweeps)
        rates = sampler.history.exchange_rate[-1]
        print("exchange_every = %d, cluster_every = %d   HMC accept rate %.3f%s" % (every, sweeps, sampler.history.accept_rate[-1],
              "" if not every else "   exchange rates " + " ".join("%.2f" % r for r in rates)))
        for k in range(K):
            e = Ensemble(ms[k], n_chains=replicas, drop=steps // 4)
            tau, tau_err, window = e.tau_int('magnetization')
            print("  kappa %.4f   chi %s   U4 %s   tau_int(m) %s (W = %d)" % (
                kappas[k], fmt_val_err(*e.susceptibility()), fmt_val_err(*e.binder()), fmt_val_err(tau, tau_err), window))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lat", default="8,8")
    ap.add_argument("--kind", choices=("affine", "rqs"), default="affine")
    ap.add_argument("--layers", type=int, default=4)
    ap.add_argument("--knots", type=int, default=16)
    ap.add_argument("--epochs", type=int, default=500)
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--nranks", type=int, default=1)
    ap.add_argument("--kappa", type=float, default=0.67)
    ap.add_argument("--m_sq", type=float, default=-4 * 0.67)
    ap.add_argument("--lambd", type=float, default=0.5)
    ap.add_argument("--transform", choices=("fft", "hartley"), default="fft",
                    help="how the spectral block filters: torch.fft, or the LDS-resident Hartley kernel (lattices up to 64 KiB per sample)")
    ap.add_argument("--hmc", action="store_true",
                    help="after the fit, print <phi^2> from model.hmc (hybrid Monte Carlo on the action) next to model.mcmc")
    ap.add_argument("--integrator", choices=sorted(INTEGRATOR_N_MD), default="leapfrog",
                    help="with --hmc: model.hmc's integration scheme (leapfrog, the second-order minimum-norm scheme, or the "
                         "fourth-order one), each at 10 force evaluations per trajectory of length 1")
    ap.add_argument("--fourier", type=float, default=None, metavar="M2",
                    help="with --hmc: model.hmc once more with the Fourier-accelerated kinetic term (fa_mass_sq=M2): acceptance, "
                         "<phi^2>, chi and tau_int(m), tau_int(phi^2) with and without acceleration")
    ap.add_argument("--fourier-path", choices=("fa", "fa_tiled", "composed"), default=None,
                    help="with --fourier: the path of the accelerated run; default: the sampler's choice (nf_phi4_hmc_fa where "
                         "the chain fits one CU, else torch ops); fa_tiled is nf_phi4_hmc_fa_tiled, for lattices beyond one CU")
    ap.add_argument("--cluster", action="store_true",
                    help="with --hmc: model.hmc once more with cluster_every=1, tau_int(m) with and without cluster sweeps; "
                         "with --ladder: the ladder once more with exchanges and cluster_every=1")
    ap.add_argument("--improved", action="store_true",
                    help="with --hmc --cluster: chi = V<m^2>, U4 and xi_2 also from the cluster-improved estimators")
    ap.add_argument("--correlator", action="store_true",
                    help="with --hmc --cluster --improved: the time-slice correlator G(t) and the effective mass along axis 0, "
                         "plain and cluster-improved (the sweeps' spectrum at all momenta)")
    ap.add_argument("--modes", action="store_true",
                    help="with --hmc --cluster --improved, two or more axes: G(p) against phat^2 at a few off-axis momenta and "
                         "m_eff of G(t; p = (1, 0, ...)), cluster-improved next to plain (nf_cluster_modes)")
    ap.add_argument("--spectrum-path", choices=("hbm",), default=None,
                    help="with --correlator: take the sweeps' spectrum with nf_cluster_spectrum_tiled (the slots in HBM), the "
                         "kernel for lattices beyond one CU's LDS; default: the one-CU kernel where it applies, else torch ops")
    ap.add_argument("--modes-path", choices=("hbm",), default=None,
                    help="with --modes: take the sweeps' modes with nf_cluster_modes_tiled (the slots in HBM), the kernel for "
                         "lattices beyond one CU's LDS; default: the one-CU kernel where it applies, else torch ops")
    ap.add_argument("--ladder", action="store_true",
                    help="no fit: a ladder of 6 kappas from --kappa down to 0.4 of it in one HMC launch per step, chi, U4 and "
                         "tau_int(m) per rung without and with replica exchange")
    a = ap.parse_args()
    lat = tuple(int(n) for n in a.lat.split(","))
    if a.ladder:
        ladder_scan(lat, a.m_sq, a.lambd, [a.kappa * (1 - 0.12 * k) for k in range(6)], cluster=a.cluster)
        return
    model = nf.Model(net_=build_net(lat, a.kind, a.layers, a.knots, a.transform), prior=NormalPrior(shape=lat),
                     action=ScalarPhi4Action(kappa=a.kappa, m_sq=a.m_sq, lambd=a.lambd))
    print("number of model parameters =", model.net_.npar)
    kw = dict(n_epochs=a.epochs, batch_size=a.batch // a.nranks, checkpoint_dict=dict(print_stride=max(1, a.epochs // 10)))
    if a.nranks > 1:
        model.device_handler.spawnprocesses(fit, a.nranks, **kw)
    else:
        model.fit(**kw)
        nf.backward_sanitychecker(model)
        if a.hmc:
            compare_with_hmc(model, cluster=a.cluster, improved=a.improved, integrator=a.integrator, correlator=a.correlator, fourier=a.fourier,
                             spectrum_path=a.spectrum_path, fourier_path=a.fourier_path, modes=a.modes,
                             modes_path=a.modes_path)


if __name__ == "__main__":
    main()
