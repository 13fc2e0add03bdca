"""``import admm_net_amd.dropin.activate_loss`` as the first line of a script: ``activate(loss=True)`` -- the shims take
precedence from here on, the ``loss`` shim (dropin/optional) among them."""
from . import _activate

_activate(loss=True)
