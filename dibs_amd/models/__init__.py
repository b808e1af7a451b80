from .graph import EdgePriorDAGDistribution, ErdosReniDAGDistribution, ScaleFreeDAGDistribution, UniformDAGDistributionRejection  # noqa: F401
from .linearGaussian import LinearGaussian, BGe  # noqa: F401
from .nonlinearGaussian import DenseNonlinearGaussian  # noqa: F401
from .discrete import BDeu, bdeu_log_marginal_numpy  # noqa: F401
