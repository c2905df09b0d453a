from ._core import Module_, ModuleList_
from ._core import MultiChannelModule_, MultiOutChannelModule_
from ._core import InvisibilityMaskWrapperModule_

from .scalar.modules import ConvAct, LinearAct, SplineNet
from .scalar.convNd import ConvNd, Conv4d
from .scalar.modules_ import DistConvertor_, Identity_, Clone_
from .scalar.modules_ import UnityDistConvertor_, PhaseDistConvertor_
from .scalar.modules_ import Expit_, Logit_, SplineNet_, ScaleNet_, SgnBiasNet_
from .scalar.modules_ import Pade11_, Pade22_, Pade32_, Tanh_, ArcTanh_

from .scalar.couplings_ import Coupling_, ShiftCoupling_, AffineCoupling_
from .scalar.couplings_ import RQSplineCoupling_, MultiRQSplineCoupling_
from .scalar.cntr_couplings_ import DirectCntrCoupling_, CntrCoupling_
from .scalar.cntr_couplings_ import CntrShiftCoupling_, CntrAffineCoupling_
from .scalar.cntr_couplings_ import CntrRQSplineCoupling_, CntrMultiRQSplineCoupling_

from .scalar.spectral_ import FFTNet_, MeanFieldNet_, PSDBlock_, IPSD, lattice_k2
