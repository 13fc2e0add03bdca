"""MI355X-native ADMM-Net forward (gfx950 HIP behind a C ABI).

Public surface mirrors the reference's admm_net.py for the forward hot path:
``ADMMNet`` and ``PhiEstADMMNet`` (same ctor / forward / state_dict keys).
Importing this package never imports the CPU oracle.
"""
from .options import Options  # noqa: F401
from .modules import ADMMNet, PhiEstADMMNet, PeakSearchLayer, PhiLayer, HLayer, GLayer, ZLayer  # noqa: F401
from . import optim  # noqa: F401
from . import order  # noqa: F401
from .order import select_targets, select_refined  # noqa: F401
from . import detect  # noqa: F401
from .detect import cfar_targets, cfar_alpha, cfar_host, cfar_relax, cfar_relax_host  # noqa: F401

__all__ = ["ADMMNet", "PhiEstADMMNet", "Options", "select_targets", "select_refined", "cfar_targets", "cfar_alpha", "cfar_host", "cfar_relax",
           "cfar_relax_host"]
