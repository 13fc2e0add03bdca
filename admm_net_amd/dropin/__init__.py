"""Drop-in shims: the reference's module names (``admm_net``, ``admm``, ``utils.peakSearchUtils``, ``utils.mathUtils``)
backed by the MI355X path, plus the mechanism that makes them win over the reference's own files.

The reference scripts are run as ``python main_for_net.py`` from the reference directory, so ``sys.path[0]`` is that
directory and a ``PYTHONPATH`` entry can never shadow its ``admm_net.py``.  Two mechanisms do:

    python -m admm_net_amd.dropin main_for_net.py [args ...]     # launcher: shims first, script directory after
    import admm_net_amd.dropin.activate                           # or: first line of a script / sitecustomize

The reference's ``loss`` module is shimmed only on request (``optional/loss.py``, the losses of admm_net_amd.losses):

    python -m admm_net_amd.dropin --hip-loss train.py [args ...]  # the flag goes BEFORE the script name
    import admm_net_amd.dropin.activate_loss                      # or: activate(loss=True)

``torch.optim.AdamW`` and ``torch.nn.utils.clip_grad_norm_`` are rebound to admm_net_amd.optim only on request as well:

    python -m admm_net_amd.dropin --hip-optim train.py [args ...] # with or without --hip-loss, in any order
    import admm_net_amd.dropin.activate_optim                     # or: activate(optim=True)

Both put this directory at the FRONT of ``sys.path``.  ``utils`` here is a package whose ``__path__`` is extended with
the script directory's own ``utils/`` so that un-shimmed submodules (``utils.plotUtils``) still resolve to the
reference's files.
"""
import os
import sys

SHIM_DIR = os.path.dirname(os.path.abspath(__file__))
REPO_ROOT = os.path.dirname(os.path.dirname(SHIM_DIR))
OPTIONAL_DIR = os.path.join(SHIM_DIR, "optional")   # shims that replace user code: opt-in only


def activate(loss=False, optim=False):
    """Put the shim directory (and the repo root, for ``import admm_net_amd``) at the front of sys.path and drop
    already-imported reference modules of the shimmed names.  ``loss=True`` adds the opt-in ``loss`` shim (dropin/optional:
    the reference's losses on HIP kernels, admm_net_amd.losses); without it ``loss`` stays the script directory's own file.
    ``optim=True`` rebinds ``torch.optim.AdamW`` and ``torch.nn.utils.clip_grad_norm_`` for this process to the wrappers of
    ``_rebind_optim`` (admm_net_amd.optim where its kernels apply, torch's originals elsewhere); without it nothing is rebound."""
    for p in (REPO_ROOT, SHIM_DIR) + ((OPTIONAL_DIR,) if loss else ()):
        if p in sys.path:
            sys.path.remove(p)
        sys.path.insert(0, p)
    for name in ("admm_net", "admm", "utils", "utils.peakSearchUtils", "utils.mathUtils") + (("loss",) if loss else ()):
        mod = sys.modules.get(name)
        f = getattr(mod, "__file__", None) or ""
        if mod is not None and not os.path.abspath(f).startswith(SHIM_DIR):
            del sys.modules[name]
    if optim:
        from . import _rebind_optim
        _rebind_optim.rebind()


_activate = activate   # importing the submodule ``dropin.activate`` rebinds the package attribute; this name stays the function
