"""``import admm_net_amd.dropin.activate_optim`` as the first line of a script: ``activate(optim=True)`` -- the shims take
precedence from here on, and ``torch.optim.AdamW`` / ``torch.nn.utils.clip_grad_norm_`` are the wrappers of ``_rebind_optim``."""
from . import _activate

_activate(optim=True)
