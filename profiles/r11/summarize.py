"""profiles/r10/summarize.py with one more class: `optim` = the optimiser kernels of csrc/optim.hip (`op_*`):
    python profiles/r11/summarize.py <dir with the rocpd .db> <out.csv> <optimisation steps in the run>
"""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location("r10_summarize", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "r10",
                                                                            "summarize.py"))
r10 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(r10)
_klass = r10.r04.klass


def klass(name):
    if "admmnet::op_" in name:
        return "optim"
    return _klass(name)


r10.r04.klass = klass

if __name__ == "__main__":
    r10.r04.main()
