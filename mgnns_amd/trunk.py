"""Row f4: the CNN trunks in front of the path, on the HIP kernels of csrc/conv_bf16.hip.

The reference builds its trunks from torchvision (MODEL:629 `models.resnet101(pretrained=...)`, MODEL:586-595
`models.__dict__['resnet50'](num_classes=365)` + the Places365 checkpoint) and keeps
`nn.Sequential(conv1, bn1, relu, maxpool, layer1, layer2, layer3, layer4)` of each (MODEL:274-294).  torchvision is a
third-party dependency that is neither vendored in the reference nor installed here, so this file restates the
published architecture (He et al. 2016 bottleneck ResNet; torchvision's "v1.5" places the stride of a stage's first block
on the 3x3 convolution) with torchvision's parameter names, which is what makes the checkpoints loadable:

  ResNet / Bottleneck   parameter containers with torchvision's state_dict surface (conv1, bn1, layer{1..4}.{i}.conv{1..3},
                        bn{1..3}, downsample.{0,1}, fc).  Their own forward() raises: there is no PyTorch compute path.
  layer_pack            the bf16 weight and fp32 bias of one (conv, bn) pair, the stem's included: 'folded' with the running
                        statistics folded in (the eval forward and frozen-statistics fine-tuning read the same tensor) or 'raw'
                        (batch-statistics fine-tuning, BatchNorm being an operator of its own there: csrc/bn_train.hip,
                        DESIGN.md 14).  One derived pack per layer, kept on the conv module, rebuilt when a tensor it derives
                        from changes and parked while a captured graph may hold its address.
  block_packs(_raw)     the layer packs of one Bottleneck plus the transposed packs its backward reads: what fine-tuning runs
                        on (ResNetFeatures.forward_train, train.TrunkStageFunction).
  run_block             the forward of one bottleneck, written once: the eval forward and both fine-tuning modes walk it with
                        their own per-layer step.
  (the stem)            with all four stages trainable the stem trains too: ResNetFeatures.forward_train(img, 4, stem=True),
                        train.TrunkStemFunction, csrc/stem_train.hip, DESIGN.md 15.
  ResNetFeatures        the reference's 8-entry nn.Sequential (same child indices -> same `object_features.4.0.conv1.weight`
                        keys), whose forward runs the HIP trunk: BatchNorm folded into bf16 weights once per version of a
                        layer's parameters, NHWC bf16 activations, every convolution an implicit GEMM on the bf16 MFMA, the
                        last one writing the [B, 2048, h, w] fp32 NCHW map the fusion path consumes.

Any module with the same attribute structure (e.g. a torchvision ResNet on a machine that has torchvision) can be
wrapped: ResNetFeatures reads the geometry (stride / padding) from the nn.Conv2d children it is given.
"""
import torch
from torch import nn

from . import ops
from .derived import derived


class _ContainerOnly(nn.Module):
    def forward(self, *a, **k):
        raise RuntimeError("%s holds parameters only: the trunk runs through mgnns_amd.trunk.ResNetFeatures "
                           "(HIP kernels); there is no PyTorch compute path" % type(self).__name__)


class Bottleneck(_ContainerOnly):
    expansion = 4

    def __init__(self, inplanes, planes, stride=1, downsample=None):
        super().__init__()
        self.conv1 = nn.Conv2d(inplanes, planes, 1, bias=False)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, stride=stride, padding=1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.conv3 = nn.Conv2d(planes, planes * self.expansion, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * self.expansion)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride


class ResNet(_ContainerOnly):
    """Bottleneck ResNet with torchvision.models.ResNet's attribute / state_dict names."""

    def __init__(self, layers, num_classes=1000):
        super().__init__()
        self.inplanes = 64
        self.conv1 = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(kernel_size=3, stride=2, padding=1)
        self.layer1 = self._make_layer(64, layers[0], 1)
        self.layer2 = self._make_layer(128, layers[1], 2)
        self.layer3 = self._make_layer(256, layers[2], 2)
        self.layer4 = self._make_layer(512, layers[3], 2)
        self.avgpool = nn.AdaptiveAvgPool2d((1, 1))
        self.fc = nn.Linear(512 * Bottleneck.expansion, num_classes)    # unused by the path (MODEL:274-294 stops at layer4)
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")

    def _make_layer(self, planes, blocks, stride):
        downsample = None
        if stride != 1 or self.inplanes != planes * Bottleneck.expansion:
            downsample = nn.Sequential(nn.Conv2d(self.inplanes, planes * Bottleneck.expansion, 1, stride=stride, bias=False),
                                       nn.BatchNorm2d(planes * Bottleneck.expansion))
        layers = [Bottleneck(self.inplanes, planes, stride, downsample)]
        self.inplanes = planes * Bottleneck.expansion
        layers += [Bottleneck(self.inplanes, planes) for _ in range(1, blocks)]
        return nn.Sequential(*layers)


def resnet50(num_classes=1000):
    """MODEL:589 `models.__dict__['resnet50'](num_classes=365)`."""
    return ResNet([3, 4, 6, 3], num_classes)


def resnet101(num_classes=1000):
    """MODEL:629 `models.resnet101(...)` (weights come from load_state_dict: there is no network here)."""
    return ResNet([3, 4, 23, 3], num_classes)


def _one(v):
    return v[0] if isinstance(v, (tuple, list)) else v


def _conv_geometry(conv, name):
    k, s, p = _one(conv.kernel_size), _one(conv.stride), _one(conv.padding)
    if (tuple(conv.kernel_size) != (k, k) or tuple(conv.stride) != (s, s) or tuple(conv.padding) != (p, p)
            or _one(conv.dilation) != 1 or conv.groups != 1 or k not in (1, 3)):
        raise ValueError("%s: only square 1x1 / 3x3, dilation 1, groups 1 convolutions are supported (got %s)" % (name, conv))
    return k, s, p


def block_layers(blk):
    """[(conv, bn)] of a bottleneck in the order its packs and gradients are kept: conv1, conv2, conv3(, downsample)."""
    layers = [(blk.conv1, blk.bn1), (blk.conv2, blk.bn2), (blk.conv3, blk.bn3)]
    if blk.downsample is not None:
        layers.append((blk.downsample[0], blk.downsample[1]))
    return layers


def layer_pack(conv, bn, kind='folded', stem=False, name="bottleneck"):
    """(wt, bias, k, stride, pad) of one convolution and its BatchNorm: the bf16 weight and fp32 bias every kernel reads.
    kind='folded': ops.conv_fold_bn with bn's running statistics folded in (the eval forward and frozen-statistics fine-tuning share
    this one tensor).  kind='raw': bf16(conv.weight) with nothing folded in and a zero bias (batch-statistics fine-tuning, where
    BatchNorm is an operator of its own).  stem=True: the 7x7 stem's [64, 160] layout.  A derived pack, kept in a store on the
    conv module and rebuilt when one of the tensors it derives from changes; the superseded one is parked while a capture lives."""
    k, s, p = (7, 2, 3) if stem else _conv_geometry(conv, name)
    if kind == 'folded':
        sources, extra = (conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var), (bn.eps,)
        build = lambda: ResNetFeatures._fold(conv, bn, stem=stem)
    else:
        sources, extra = (conv.weight,), ()
        build = lambda: ops.conv_fold_bn(conv.weight.detach().contiguous(), None, None, stem=stem)
    store = conv.__dict__.setdefault("_packs", {})
    wt, bias = derived(store, "stem." + kind if stem else kind, sources, build, extra=extra, park=ops.retire)
    return wt, bias, k, s, p


def _train_packs(blk, kind):
    out = []
    for conv, bn in block_layers(blk):
        if conv.bias is not None:
            raise NotImplementedError("trunk fine-tuning: convolutions with a bias are not supported (torchvision's have none)")
        wt, bias, k, s, p = layer_pack(conv, bn, kind)
        # the data gradient's transposed pack derives from wt alone, in a slot of its own: only a backward asks for it
        wT = derived(conv._packs, kind + ".T", (wt,), lambda: ops.conv_transpose_pack(wt, k), park=ops.retire)
        out.append((wt, bias, wT, k, s, p))
    return out


def block_packs(blk):
    """[(wt, bias, wT, k, stride, pad)] per block_layers(blk) for frozen-statistics fine-tuning: the folded layer_pack of each layer
    and its transposed pack (ops.conv_transpose_pack), which the data gradient reads."""
    return _train_packs(blk, 'folded')


def block_packs_raw(blk):
    """[(wt, zero bias, wT, k, stride, pad)] per block_layers(blk) for batch-statistics fine-tuning: the raw
    layer_pack of each layer and its transposed pack."""
    return _train_packs(blk, 'raw')


def run_block(y, down, step, last=False):
    """The forward of one bottleneck, for every mode: (relu(layer3(layer2(layer1(y))) + idn), idn) with idn = the downsample layer
    of y if the block has one (`down`), else y.  step(j, x, relu=, residual=, out_nchw_f32=) runs layer j of block_layers on x and
    returns its activation; whatever a backward needs, the step records.  last: the output is the fp32 NCHW map.  Nothing but the
    running activation is held here: o1 is released before the third layer allocates its output."""
    idn = step(3, y, relu=False) if down else y
    o = step(0, y)
    o = step(1, o)
    return step(2, o, residual=idn, out_nchw_f32=last), idn


def conv_step(packs):
    """run_block's step that is one launch: layer j's convolution on packs[j] (layer_pack's or block_packs') with its bias,
    residual and ReLU -- the whole layer on a folded pack."""
    return lambda j, x, **kw: ops.conv_bf16_nhwc(x, packs[j][0], packs[j][1], *packs[j][-3:], **kw)


class ResNetFeatures(nn.Sequential):
    """MODEL:274-294 `nn.Sequential(conv1, bn1, relu, maxpool, layer1..layer4)` with a HIP forward.

    forward(img [B,3,H,W] fp32 NCHW on the GPU) -> [B, 2048, H/32, W/32] fp32 NCHW (eval mode only)."""

    def __init__(self, m):
        super().__init__(m.conv1, m.bn1, m.relu, m.maxpool, m.layer1, m.layer2, m.layer3, m.layer4)
        c, mp = m.conv1, m.maxpool
        if (tuple(c.kernel_size), tuple(c.stride), tuple(c.padding), c.in_channels, c.out_channels) != ((7, 7), (2, 2), (3, 3), 3, 64):
            raise ValueError("trunk stem must be Conv2d(3, 64, 7, stride 2, padding 3), got %s" % (c,))
        if (_one(mp.kernel_size), _one(mp.stride), _one(mp.padding)) != (3, 2, 1) or getattr(mp, "ceil_mode", False):
            raise ValueError("trunk max-pool must be MaxPool2d(3, 2, 1), got %s" % (mp,))

    @staticmethod
    def _fold(conv, bn, stem=False):
        return ops.conv_fold_bn(conv.weight.detach().contiguous(), None if conv.bias is None else conv.bias.detach(),
                                (bn.weight.detach(), bn.bias.detach(), bn.running_mean, bn.running_var, bn.eps), stem=stem)

    def _prepare(self, stop=8):
        """(the stem's folded pack, [[layer_pack per block_layers(blk)] per block of the stages self[4:stop]]): the eval plan.
        Every entry is the layer's own derived pack, so a changed parameter refolds its layer and nothing else."""
        blocks = []
        for li in range(4, stop):
            for bi, blk in enumerate(self[li]):
                name = "%d.%d" % (li, bi)
                blocks.append([layer_pack(conv, bn, name=name + ".downsample" if j == 3 else name)
                               for j, (conv, bn) in enumerate(block_layers(blk))])
        return layer_pack(self[0], self[1], stem=True), blocks

    def _eval(self, img, stop=8):
        """The stem, the max-pool and the stages self[4:stop] on the folded packs -> bf16 NHWC, or after layer4 the fp32 NCHW map."""
        stem, blocks = self._prepare(stop)
        y = ops.stem_conv7(img.contiguous(), *stem[:2])
        y = ops.maxpool3x3s2_nhwc(y)
        for i, packs in enumerate(blocks):
            y = run_block(y, len(packs) == 4, conv_step(packs), last=stop == 8 and i == len(blocks) - 1)[0]
        return y

    def forward_train(self, img, stages=1, batchnorm='frozen', stem=False):
        """Fine-tuning forward: img [B,3,H,W] -> the [B,2048,h,w] fp32 map under autograd, with gradients for the parameters of
        the last `stages` bottleneck stages that require one.  The stem, the max-pool and the stages below run as in forward(),
        without a graph and with their running statistics, so the module itself must be in eval mode (model.unfreeze_trunks()
        puts it there).  batchnorm='frozen': the trainable stages keep their running statistics too.  batchnorm='batch': their
        BatchNorm layers normalise with the statistics of the batch, move running_mean / running_var / num_batches_tracked and
        are differentiated through the statistics (train.TrunkStageFunction, either way).
        stem=True (needs stages=4): the stem trains too -- conv1.weight, bn1.weight and bn1.bias get gradients if they require one
        (train.TrunkStemFunction), and in 'batch' mode bn1 uses and moves batch statistics like every other BatchNorm.  The image
        itself never gets a gradient."""
        from . import train as _train
        if batchnorm not in _train.TRUNK_BATCHNORM_MODES:
            raise ValueError("batchnorm must be one of %s, got %r" % (_train.TRUNK_BATCHNORM_MODES, batchnorm))
        if self.training:
            raise RuntimeError("ResNetFeatures.forward_train keeps BatchNorm's running statistics (frozen-statistics fine-tuning): "
                               "call .eval() on the trunk, or model.unfreeze_trunks()")
        if not 1 <= int(stages) <= 4:
            raise ValueError("stages must be 1..4, got %r" % (stages,))
        if stem and int(stages) != 4:
            raise ValueError("stem=True trains the stem below four trainable stages: it needs stages=4, got stages=%r" % (stages,))
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError("trunk input must be [B, 3, H, W], got %s" % (tuple(img.shape),))
        if not img.is_cuda:
            raise RuntimeError("img is on %s: mgnns_amd operators run on the GPU only (no CPU path)" % img.device)
        first = 8 - int(stages)
        if stem:
            y = _train.trunk_stem_forward(self[0], self[1], img, batchnorm=batchnorm)
        else:
            with torch.no_grad():
                y = self._eval(img.detach(), first)
        return _train.trunk_stage_forward([self[li] for li in range(first, 8)], y, batchnorm=batchnorm)

    def forward(self, img):
        if self.training:
            raise RuntimeError("ResNetFeatures: eval-mode forward only on the HIP path (BatchNorm uses running statistics); call .eval()")
        if img.dim() != 4 or img.shape[1] != 3:
            raise ValueError("trunk input must be [B, 3, H, W], got %s" % (tuple(img.shape),))
        return self._eval(img)


def features_flops(feats, size):
    """Algorithmic FLOPs (2 x MACs of the stem and of every bottleneck convolution) of ONE size x size image through a
    ResNetFeatures -- the figure the trunk's MFMA utilisation is quoted on (62.4 GFLOP for ResNet-101 at 448)."""
    h = (size - 1) // 2 + 1
    total = 2 * 64 * 147 * h * h
    h = (h - 1) // 2 + 1
    for li in range(4, 8):
        for blk in feats[li]:
            hin = h
            for conv in (blk.conv1, blk.conv2, blk.conv3):
                k, s, p = _one(conv.kernel_size), _one(conv.stride), _one(conv.padding)
                h = (h + 2 * p - k) // s + 1
                total += 2 * conv.out_channels * conv.in_channels * k * k * h * h
            if blk.downsample is not None:
                d = blk.downsample[0]
                ho = (hin - 1) // _one(d.stride) + 1
                total += 2 * d.out_channels * d.in_channels * ho * ho
    return total
