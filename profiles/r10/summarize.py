"""profiles/r04/summarize.py with two more classes (route "native"): `train_hlayer` = the H-layer kernels and the batch-reduced
product of csrc/train_hlayer.hip, `train_head` = the head kernels and products of csrc/train_head.hip:
    python profiles/r10/summarize.py <dir with the rocpd .db> <out.csv> <optimisation steps in the run>
"""
import importlib.util
import os

_spec = importlib.util.spec_from_file_location("r04_summarize", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "r04",
                                                                            "summarize.py"))
r04 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(r04)
_klass = r04.klass


def klass(name):
    if "admmnet::hd_" in name or "admmnet::hb_" in name or "bp_kernel<admmnet::HbTable>" in name:
        return "train_head"
    if "admmnet::th_" in name or "admmnet::bp_" in name:
        return "train_hlayer"
    return _klass(name)


r04.klass = klass

if __name__ == "__main__":
    r04.main()
