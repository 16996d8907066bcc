"""``Demix.MotionCorrect`` (the reference's module name); the implementation lives in dnmf_amd."""
from dnmf_amd.Demix.MotionCorrect import MotionCorrect, high_pass_filter_space  # noqa: F401
