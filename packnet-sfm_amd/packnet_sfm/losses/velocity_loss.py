"""Velocity supervision on a fused MI355X kernel.

Drop-in for the reference's packnet_sfm/losses/velocity_loss.py: `VelocityLoss(**kwargs)`, `forward(pred_pose, gt_pose_context)` ->
{'loss': [1], 'metrics': {'velocity_loss'}}.  The loss compares the LENGTHS of the predicted and the ground-truth translations,
L = (1/J) sum_j mean_b | |t_pred[j,b]| - |t_gt[j,b]| |, which is what ties a self-supervised model to metres.  The reference spends
about 20 ATen launches on it each way; here it is one launch each way for all J contexts (csrc/velocity.h), bit-reproducible.
"""
from packnet_sfm.hip import functional as HF
from packnet_sfm.losses.loss_base import LossBase


class VelocityLoss(LossBase):
    def __init__(self, **kwargs):
        super().__init__()

    def forward(self, pred_pose, gt_pose_context, weight=1.0, loss_in=None, **kwargs):
        """
        pred_pose: list of J Pose (or [B,4,4] tensors), target -> context; gt_pose_context: list of J [B,4,4] ground-truth transforms
        (float32, or float64 as datasets deliver them).  Returns {'loss': [1], 'metrics': {'velocity_loss'}}.

        With `loss_in` (a one-element loss tensor) the same launch also forms loss_in + weight * loss, returned under 'total' in
        loss_in's shape: the gradient then flows through 'total' and 'loss' is the plain value.
        """
        assert len(pred_pose) == len(gt_pose_context), \
            'VelocityLoss: {} predicted poses for {} ground-truth poses'.format(len(pred_pose), len(gt_pose_context))
        mats = [p.mat if hasattr(p, 'mat') else p for p in pred_pose]
        gts = [g.mat if hasattr(g, 'mat') else g for g in gt_pose_context]
        if loss_in is None:
            loss, _ = HF.velocity_loss(mats, gts)                    # weight 1: the total IS the loss, and carries the gradient
            self.add_metric('velocity_loss', loss)
            return {'loss': loss.unsqueeze(0), 'metrics': self.metrics}
        total, loss = HF.velocity_loss(mats, gts, weight=weight, loss_in=loss_in)
        self.add_metric('velocity_loss', loss)
        return {'loss': loss.unsqueeze(0), 'total': total.reshape(loss_in.shape), 'metrics': self.metrics}


# names of the reference's module of the same path that the hot path does not re-implement (packnet_sfm/_merge.py)
from packnet_sfm._merge import reference_fallback as _reference_fallback  # noqa: E402
__getattr__ = _reference_fallback(__name__, __file__)
