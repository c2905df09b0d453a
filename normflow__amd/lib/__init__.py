from .stats import Resampler, estimate_logz, fmt_val_err
from .observables import measure, Measurement, Ensemble, measure_improved, ImprovedMeasurement, ImprovedEnsemble, measure_modes, correlator_modes
