from .mcmc import MCMCSampler, BlockedMCMCSampler, MCMCHistory, Metropolis, ModifiedMetropolis
from .hmc import HMCSampler, HMCHistory
from .ladder import LadderHMCSampler, LadderHistory
from .cluster import cluster_sweep
