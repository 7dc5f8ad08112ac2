"""diral_amd - MI355X-native batched V2V resource-allocation environment.

The one data-parallel hot path of gundoganalperen/DIRAL (envs/test_env.py +
network.py + vehicle.py: the env step) as hand-written HIP for gfx950 behind a
C-ABI (include/diral_env.h), with a host-side mirror of the reference's env
interface.  See DESIGN.md.
"""
from .config import (ConfigError, EnvConfig, StateConfig, STEP_DESIGN, STEP_MY_STEP, STEP_MY_STEP_CH,
                     bench_config, c2_config)

__all__ = ["EnvConfig", "StateConfig", "ConfigError", "VecV2VEnv", "StreamedVecEnv", "TestEnv", "QPolicy", "ReplayMemory", "QLoss", "QNet", "LSTM", "DRQNet",
           "bench_config", "c2_config", "STEP_MY_STEP", "STEP_MY_STEP_CH", "STEP_DESIGN"]


def __getattr__(name):
    # torch-dependent classes are imported lazily so config/oracle tooling can
    # be used without touching the GPU stack
    if name == "VecV2VEnv":
        from .vec_env import VecV2VEnv
        return VecV2VEnv
    if name == "StreamedVecEnv":
        from .streamed import StreamedVecEnv
        return StreamedVecEnv
    if name == "QPolicy":
        from .qpolicy import QPolicy
        return QPolicy
    if name == "ReplayMemory":
        from .memory import ReplayMemory
        return ReplayMemory
    if name == "QLoss":
        from .qloss import QLoss
        return QLoss
    if name == "QNet":
        from .qnet import QNet
        return QNet
    if name in ("LSTM", "DRQNet"):
        from . import lstm
        return getattr(lstm, name)
    if name == "TestEnv":
        from .compat import TestEnv
        return TestEnv
    raise AttributeError(name)
