"""gym_lowcostrobot_amd -- MI355X-native batched simulator for the low-cost 6-DoF arm + cube tasks.

Drop-in for the hot path of perezjln/gym-lowcostrobot (batched reset/step of the five cube tasks);
see DESIGN.md / INTEGRATION.md.  Requires liblcr_hip.so (python -m gym_lowcostrobot_amd.build) and a
gfx950 GPU: there is no CPU fallback.
"""
__version__ = "0.1.0"

from .vecsim import VecSim  # noqa: F401
from ._capi import LookSampler, LookVariant, WristCamera  # noqa: F401,E402
from . import envs  # noqa: F401,E402
from .envs import register_envs  # noqa: F401,E402
from .vecenv import LowCostRobotVecEnv, LowCostRobotVectorEnv  # noqa: F401,E402



def default_look_variant():
    """the look every frame has without look_variants (lcr_look_variant_default): scene cameras unmoved, fovy 45, the scene's floor, sky, light and arm colours"""
    return LookVariant.from_any({})


def default_wrist_camera():
    """the default mount of VecSim(wrist_camera=True) (lcr_wrist_camera_default) as a dict: link 5, above the gripper body, looking 25 degrees down towards the end-effector site"""
    return WristCamera.from_any(True).as_dict()


register_envs()
