"""Model factory and init (utils/model_utils.py:12-140), same signatures."""
from __future__ import annotations

import sys

import torch
from torch.nn import init

from .discriminator import (BaseDiscNet, DeepConvDiscNet, PointDiscNet, PointwiseDiscNet,
                            ShapeDiscNet, StackDiscNet)
from .pointnet import PointNetCls


def init_net(net, device, init_type, init_gain=1.0):
    """utils/model_utils.py:12-25: move to device, then init_weights."""
    net.to(device)
    if init_type is None:
        return net
    init_weights(net, init_type, init_gain=init_gain)
    return net


# weight initialisers by init_type (utils/model_utils.py:27-58); biases go to 0
_WEIGHT_INIT = {
    "normal": lambda w, gain: init.normal_(w, 0.0, gain),
    "xavier": lambda w, gain: init.xavier_normal_(w, gain=gain),
    "kaiming": lambda w, gain: init.kaiming_normal_(w, a=0, mode="fan_in"),
    "orthogonal": lambda w, gain: init.orthogonal_(w, gain=gain),
}


def init_weights(net, init_type, init_gain=1.0, verbose=True):
    """Initialise every Conv*/Linear weight of `net` by `init_type` and zero its
    bias; BatchNorm2d weights ~ N(1, init_gain), biases 0 (interface and
    distributions of utils/model_utils.py:27-58).  Leaf modules are visited in
    registration order, the order Module.apply reaches them, so a seeded torch
    RNG gives the reference's weights."""
    if verbose:
        print("initialize network with %s" % init_type)
    if init_type is None:
        return net
    fill = _WEIGHT_INIT.get(init_type)
    for mod in net.modules():
        kind = type(mod).__name__
        if ("Conv" in kind or "Linear" in kind) and hasattr(mod, "weight"):
            if fill is None:
                raise NotImplementedError("initialization method [%s] is not implemented" % init_type)
            fill(mod.weight.data, init_gain)
            if getattr(mod, "bias", None) is not None:
                mod.bias.data.zero_()
        elif "BatchNorm2d" in kind:
            init.normal_(mod.weight.data, 1.0, init_gain)
            mod.bias.data.zero_()
    return net


def load_models(mode, device, args):
    """utils/model_utils.py:60-140 for the hot path's modes 'cls' and 'disc', the
    segmentation row's 'seg', its per-point discriminator 'disc_seg', the
    stacked shape discriminator 'disc_stack', the regularised generator
    'seg_regu' and the dual discriminator 'disc_dual' (:116-133), which returns
    the tuple (shared, shape, point) of BaseDiscNet, ShapeDiscNet, PointDiscNet."""
    if mode == "cls":
        model = PointNetCls(k=40, feature_transform=False).to(device)
        try:
            if getattr(args, "checkpoint", None):
                print("===============================")
                print("Loading pretrained cls model ...")
                print("===============================")
                model.load_state_dict(torch.load(args.checkpoint, map_location=device,
                                                 weights_only=True))
        except Exception as e:  # reference: print and exit(0) (:77-79)
            print(e)
            sys.exit(0)
    elif mode == "disc":
        model = DeepConvDiscNet(input_dim=args.disc_indim, output_dim=1)
        model = init_net(model, device, init_type=args.init_disc)
    elif mode == "seg":  # :80-90, PointNetSeg
        from .seg import PointNetSeg
        model = PointNetSeg(NUM_SEG_CLASSES=50)
        model = init_net(model, device, init_type=args.init_disc)
        if getattr(args, "checkpoint", None):
            print("Loading pretrained cls model ...")
            model.load_state_dict(torch.load(args.checkpoint, map_location=device,
                                             weights_only=True))
    elif mode == "disc_seg":  # :113-115, PointwiseDiscNet (run_training_seg's D)
        model = PointwiseDiscNet(input_pts=args.input_pts, input_dim=args.disc_indim)
        model = init_net(model, device, init_type=args.init_disc)
    elif mode == "disc_stack":  # StackDiscNet (run_training_seg_stack's D)
        model = StackDiscNet(input_pts=args.input_pts, input_dim=args.disc_indim, num_shapes=16)
        model = init_net(model, device, init_type=args.init_disc)
    elif mode == "seg_regu":  # :92-103, PointNetSeg_regulization, initialised like a discriminator
        from .seg import PointNetSeg_regulization
        model = PointNetSeg_regulization(NUM_SEG_CLASSES=50)
        model = init_net(model, device, init_type=args.init_disc)
        if getattr(args, "checkpoint", None):
            print("Loading pretrained cls model ...")
            model.load_state_dict(torch.load(args.checkpoint, map_location=device,
                                             weights_only=True))
    elif mode == "disc_dual":  # :116-133, run_training_seg_dual's three nets
        shared = BaseDiscNet(input_pts=args.input_pts, input_dim=args.disc_indim, output_dim=256)
        shape = ShapeDiscNet(shared_output_dim=256, num_shapes=16)
        point = PointDiscNet(shared_output_dim=256, input_pts=args.input_pts)
        return tuple(init_net(m, device, init_type=args.init_disc) for m in (shared, shape, point))
    else:
        raise ValueError("Invalid mode {}!".format(mode))
    return model
