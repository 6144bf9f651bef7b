"""VelSupModel: the self-supervised model plus velocity supervision, which makes its depth scale-aware (contract of the reference's
packnet_sfm/models/VelSupModel.py: `velocity_loss_weight`, batch key 'pose_context', train requirement 'gt_pose').  The reference's
own class cannot be constructed (it indexes the list of train requirements with a string); this one can."""
from packnet_sfm.losses.velocity_loss import VelocityLoss
from packnet_sfm.models.SelfSupModel import SelfSupModel


class VelSupModel(SelfSupModel):
    """
    velocity_loss_weight : float   w: loss = self-supervised + w * velocity loss
    kwargs                         options of SelfSupModel and its loss
    """

    def __init__(self, velocity_loss_weight=0.1, **kwargs):
        super().__init__(**kwargs)
        self._velocity_loss = VelocityLoss(**kwargs)
        self.velocity_loss_weight = velocity_loss_weight
        self._train_requirements.append('gt_pose')

    def forward(self, batch, return_logs=False, progress=0.0):
        if not self.training:                           # evaluation: predictions only
            return super().forward(batch, return_logs=return_logs, progress=progress)
        if 'pose_context' not in batch:
            raise KeyError("VelSupModel needs ground-truth poses to train: the batch has no 'pose_context' "
                           "(the model's train requirement 'gt_pose')")
        output = super().forward(batch, return_logs=return_logs, progress=progress)
        # one launch: the velocity loss of all contexts AND loss + w * velocity loss
        velocity = self._velocity_loss(output['poses'], batch['pose_context'], weight=self.velocity_loss_weight,
                                       loss_in=output['loss'])
        output['loss'] = velocity['total']
        output['metrics'] = {**output['metrics'], **velocity['metrics']}
        return output


# names of the reference's module of the same path that the hot path does not re-implement (packnet_sfm/_merge.py)
from packnet_sfm._merge import reference_fallback as _reference_fallback  # noqa: E402
__getattr__ = _reference_fallback(__name__, __file__)
