from .mcmc import MCMCSampler, BlockedMCMCSampler, MCMCHistory, Metropolis, ModifiedMetropolis
from .hmc import HMCSampler, HMCHistory
