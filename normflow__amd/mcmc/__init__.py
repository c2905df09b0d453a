from .mcmc import MCMCSampler, BlockedMCMCSampler, MCMCHistory, Metropolis, ModifiedMetropolis
from .hmc import HMCSampler, HMCHistory
from .ladder import LadderHMCSampler, LadderHistory
