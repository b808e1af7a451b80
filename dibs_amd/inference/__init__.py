from .dibs import DiBS  # noqa: F401
from .svgd import MarginalDiBS, JointDiBS  # noqa: F401
from .batch import sample_batch  # noqa: F401
from .sweep import sample_sweep  # noqa: F401
from .chains import sample_chains  # noqa: F401
from .joint_batch import sample_joint_batch  # noqa: F401
from .joint_sweep import sample_joint_sweep  # noqa: F401
