"""The part of the reference's `utils/train_module.py` that evaluation needs: `loss_fn`, the regression losses of the
flow-matching models (l2, l1, huber, smooth_l1, log_cosh), on the device through codlad_fm_terms.  Training itself is out of
scope."""
from ..diffusion_and_flow.flow import LOSS_TYPES, batch_loss, loss_fn  # noqa: F401
