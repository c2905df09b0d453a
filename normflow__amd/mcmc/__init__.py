from .mcmc import MCMCSampler, BlockedMCMCSampler, MCMCHistory, Metropolis, ModifiedMetropolis
