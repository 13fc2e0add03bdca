"""``python -m admm_net_amd.dropin [--hip-loss] [--hip-optim] script.py [args ...]``: run one of the reference's scripts
(main_for_net.py, test/test_time_net.py, main.py, test/test_time_admm.py, trainPhi.py ...) unchanged on the MI355X path.

The script runs as ``__main__`` with the import order  shims -> repo root -> the script's own directory -> the rest,
exactly what ``python script.py`` gives except that the shims come first.  Nothing is exec'ed: the script runs
inside this interpreter (runpy), so a GPU that is already initialised is not an issue.
The flags go before the script name, in any order; everything after the script name goes to the script.
``--hip-loss`` also shims the reference's ``loss`` module, which otherwise stays the script directory's own file.
``--hip-optim`` rebinds ``torch.optim.AdamW`` and ``torch.nn.utils.clip_grad_norm_`` to admm_net_amd.optim for this process.
"""
import os
import runpy
import sys

from . import activate

FLAGS = {"--hip-loss": "loss", "--hip-optim": "optim"}


def main():
    args = sys.argv[1:]
    on = {}
    while args and args[0] in FLAGS:
        on[FLAGS[args[0]]] = True
        args = args[1:]
    if not args:
        sys.exit("usage: python -m admm_net_amd.dropin [--hip-loss] [--hip-optim] script.py [args ...]")
    script = os.path.abspath(args[0])
    sys.argv = [script] + args[1:]
    here = os.path.dirname(script)
    if here in sys.path:
        sys.path.remove(here)
    sys.path.insert(0, here)            # what `python script.py` would have put first ...
    activate(**on)                      # ... and the shims in front of it
    runpy.run_path(script, run_name="__main__")


if __name__ == "__main__":
    main()
