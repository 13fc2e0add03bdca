"""Opt-in drop-in for the reference's ``loss`` module: its three public names on the kernels of csrc/loss.hip, and
``PhiSpectralLoss`` (csrc/loss_spectrum.hip) and ``SetANMLoss`` (csrc/loss_set.hip) beside them.  This directory
goes on ``sys.path`` only with ``dropin.activate(loss=True)`` / ``--hip-loss`` / ``import admm_net_amd.dropin.activate_loss``."""
from admm_net_amd.losses import BasicANMLoss, PhiAlignmentLoss, PhiSpectralLoss, SetANMLoss, basic_parameter_loss  # noqa: F401
