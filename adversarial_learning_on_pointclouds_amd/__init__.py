"""MI355X-native PointNet adversarial-training hot path (gfx950 HIP kernels).

Drop-in counterparts of the reference's models and training loop
(YiruS/Adversarial_Learning_on_PointClouds): PointNetCls / PointNetfeat
(models/pointnet.py), DeepConvDiscNet (models/discriminator.py), load_models
(utils/model_utils.py), make_D_label (utils/utils.py), ImagePool
(utils/image_pool.py), run_training / run_testing (utils/trainer.py), plus the
fused native step AdvTrainStep; PointNetSeg (models/pointnet.py:261-317) with
its native training step SegTrainStep; PointwiseDiscNet
(models/discriminator.py:53-79) and the adversarial segmentation step
SegAdvTrainStep (run_training_seg, and run_training_seg_semi with its
pseudo-label term); StackDiscNet (models/discriminator.py:139-175) and
SegStackTrainStep (run_training_seg_stack); PointNetSeg_regulization
(models/pointnet.py:205-259) and SegStackReguTrainStep
(run_training_seg_stack_regulization), both with the pseudo-label term
(semi=True: run_training_seg_stack_semi,
run_training_seg_stack_regulization_semi); BaseDiscNet / ShapeDiscNet /
PointDiscNet (models/discriminator.py:82-137) and SegDualTrainStep
(run_training_seg_dual); run_training_semi; the HDF5 datasets of
dataset/modelNetData.py and dataset/shapeNetData.py without h5py, with a
device-resident batch loader (dataset.DeviceCloudLoader) and native test
passes over it (evaluate.ClsEvaluator / SegEvaluator).  All compute runs in
libpcadv.so (C ABI in include/pcadv.h); there is no CPU fallback.
"""
from . import _lib  # noqa: E402
from ._lib import use_stream_graph_dispatch  # noqa: E402
from .discriminator import (BaseDiscNet, DeepConvDiscNet, PointDiscNet,  # noqa: E402
                            PointwiseDiscNet, ShapeDiscNet, StackDiscNet)
from .evaluate import ClsEvaluator, SegEvaluator  # noqa: E402
from .pointnet import PointNetCls, PointNetfeat, STN3d, STNkd, feature_transform_regularizer  # noqa: E402,E501
from .seg import (PointNetSeg, PointNetSeg_regulization, SegAdvTrainStep,  # noqa: E402
                  SegDualTrainStep, SegStackReguTrainStep, SegStackTrainStep, SegTrainStep)
from .step import AdvTrainStep  # noqa: E402

__all__ = ["PointNetCls", "PointNetfeat", "STN3d", "STNkd", "DeepConvDiscNet",
           "feature_transform_regularizer", "AdvTrainStep", "PointNetSeg", "SegTrainStep",
           "PointwiseDiscNet", "SegAdvTrainStep", "StackDiscNet", "SegStackTrainStep",
           "PointNetSeg_regulization", "SegStackReguTrainStep", "BaseDiscNet",
           "ShapeDiscNet", "PointDiscNet", "SegDualTrainStep",
           "ClsEvaluator", "SegEvaluator"]
__version__ = "0.1.0"
