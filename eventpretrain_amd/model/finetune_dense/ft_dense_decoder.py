"""Dense-prediction decoder heads (reference model/finetune_dense/ft_dense_decoder.py): UPerNet (pyramid pooling + FPN) as the decode
head, FCN as the auxiliary head. Same constructors, factories, attribute names and therefore state-dict keys as the reference
(`psp_modules.{i}.1.{conv_layer,norm_layer}.*`, `psp_bottleneck.*`, `lateral_convs.{i}.*`, `fpn_convs.{i}.*`, `fpn_bottleneck.*`,
`conv_dense.*`, `convs.{i}.*`, `conv_cat.*`): nn.Conv2d / nn.BatchNorm2d are parameter containers only. The math runs on token-major
maps [B*H*W, C] through ops.ConvBNFn, AdaptivePoolFn, UpsampleBilinearFn, ChannelDropoutFn and DenseClsFn (csrc/dense.hip + the GEMM);
a torch.cat(dim=1) of the reference is one buffer whose producers write their channel slices (ops.CatFn). A map that is a permuted view
of a contiguous token tensor (utils.reshape.emb2patch_frame) is consumed where it lies."""
import torch
import torch.nn as nn

from ... import ops


def to_map(x):
    """(B, C, H, W) -> token-major [B*H*W, C] (a view when x is a permuted token tensor), B, H, W."""
    B, C, H, W = x.shape
    t = x.permute(0, 2, 3, 1)
    if not t.is_contiguous():
        t = t.contiguous()
    return t.view(B * H * W, C), B, H, W


def from_map(m, B, H, W):
    """Token-major [B*H*W, C] (rows possibly strided) -> an NCHW-shaped view."""
    return m.view(B, H, W, m.shape[1]).permute(0, 3, 1, 2)


class ConvModule(nn.Module):
    """Conv2d (with bias) -> BatchNorm2d -> ReLU; kernel 1 or 3, padding k // 2."""

    def __init__(self, in_channels, out_channels, kernel_size, padding=0, norm_layer=nn.BatchNorm2d, act_layer=None):
        super().__init__()
        self.conv_layer = nn.Conv2d(in_channels, out_channels, kernel_size=kernel_size, padding=padding)
        self.norm_layer = norm_layer(out_channels)
        self.act_layer = nn.ReLU(inplace=True) if act_layer is None else act_layer

    def on_map(self, m, B, H, W, out=None):
        return ops.conv_bn_map(m, self.conv_layer, self.norm_layer, B, H, W, relu=True, out=out)

    def forward(self, x):
        m, B, H, W = to_map(x)
        return from_map(self.on_map(m, B, H, W), B, H, W)


class BaseDecodeHead(nn.Module):
    def __init__(self, args, in_channels, channels, out_channels, dropout_ratio=0.1, in_index=-1, input_transform="multiple_select"):
        super().__init__()
        self.in_channels = in_channels
        self.channels = channels
        self.out_channels = out_channels
        self.sample_mode = args.sample_mode
        if self.sample_mode != "bilinear":
            raise NotImplementedError(f"sample_mode {self.sample_mode!r}: only 'bilinear' (what both of the reference's entry scripts set)")
        self.dropout_ratio = dropout_ratio
        self.dropout = nn.Dropout2d(dropout_ratio) if dropout_ratio > 0 else None
        self.in_index = in_index
        self.input_transform = input_transform
        self.conv_dense = nn.Conv2d(channels, self.out_channels, kernel_size=1)
        self.given_keep = None        # tests: a uint8 [B, channels] keep mask to use instead of a drawn one
        self.last_keep = None         # the uint8 [B * channels] keep mask of the last training-mode call

    def cls_dense_map(self, feat, B, H, W):
        """Channel dropout (training mode) and the per-pixel classifier on a map -> float32 [B*H*W, out_channels]."""
        if self.dropout is not None and self.training:
            scale, self.last_keep = ops.draw_channel_scale(B, self.channels, self.dropout_ratio, feat.device, keep=self.given_keep)
            feat = ops.ChannelDropoutFn.apply(feat, scale, H * W)
        return ops.DenseClsFn.apply(feat, self.conv_dense.weight, self.conv_dense.bias)

    def forward(self, inputs):
        feat, B, H, W = self._forward_feature_map(inputs)
        return from_map(self.cls_dense_map(feat, B, H, W), B, H, W)

    def _forward_feature(self, inputs):
        feat, B, H, W = self._forward_feature_map(inputs)
        return from_map(feat, B, H, W)


class PPM(nn.ModuleList):
    """Pooling pyramid of PSPNet: per scale AdaptiveAvgPool2d(s) -> 1x1 ConvModule -> resize back."""

    def __init__(self, sample_mode, pool_scales, in_channels, channels, **kwargs):
        super().__init__()
        self.pool_scales = pool_scales
        self.in_channels = in_channels
        self.channels = channels
        self.sample_mode = sample_mode
        for pool_scale in pool_scales:
            self.append(nn.Sequential(nn.AdaptiveAvgPool2d(pool_scale), ConvModule(self.in_channels, self.channels, 1, **kwargs)))

    def on_map(self, m, B, H, W, outs=None):
        """The resized branch outputs; outs[i] = (buf, off): branch i writes its slice of a concat buffer."""
        res = []
        for i, (s, ppm) in enumerate(zip(self.pool_scales, self)):
            p = ops.AdaptivePoolFn.apply(m, B, H, W, s)
            c = ppm[1].on_map(p, B, s, s)
            res.append(ops.resize_map(c, B, s, s, H, W, self.sample_mode, None if outs is None else outs[i]))
        return res

    def forward(self, x):
        m, B, H, W = to_map(x)
        return [from_map(o, B, H, W) for o in self.on_map(m, B, H, W)]


def _concat_buffer(R, width, device):
    return torch.empty(R, width, dtype=ops.get_compute_dtype(), device=device)


class UPerHead(BaseDecodeHead):
    def __init__(self, pool_scales=(1, 2, 3, 6), in_index=-1, **kwargs):
        super().__init__(**kwargs)
        self.in_index = in_index
        self.psp_modules = PPM(self.sample_mode, pool_scales, self.in_channels[-1], self.channels)
        self.psp_bottleneck = ConvModule(self.in_channels[-1] + len(pool_scales) * self.channels, self.channels, 3, padding=1)
        self.lateral_convs = nn.ModuleList()
        self.fpn_convs = nn.ModuleList()
        for in_channels in self.in_channels[:-1]:       # the top level goes through the pyramid pooling instead
            self.lateral_convs.append(ConvModule(in_channels, self.channels, 1))
            self.fpn_convs.append(ConvModule(self.channels, self.channels, 3, padding=1))
        self.fpn_bottleneck = ConvModule(len(self.in_channels) * self.channels, self.channels, 3, padding=1)

    def psp_forward_map(self, m, B, H, W):
        ch, cin = self.channels, self.in_channels[-1]
        buf = _concat_buffer(B * H * W, cin + len(self.psp_modules) * ch, m.device)
        parts = [ops.MapCopyFn.apply(m, buf.dtype, (buf, 0))]
        parts += self.psp_modules.on_map(m, B, H, W, [(buf, cin + i * ch) for i in range(len(self.psp_modules))])
        return self.psp_bottleneck.on_map(ops.CatFn.apply((buf,), *parts), B, H, W)

    def _forward_feature_map(self, inputs):
        maps = [to_map(x) for x in inputs]
        n, ch = len(maps), self.channels
        B = maps[0][1]
        size = [(H, W) for _, _, H, W in maps]
        laterals = [conv.on_map(maps[i][0], B, *size[i]) for i, conv in enumerate(self.lateral_convs)]
        laterals.append(self.psp_forward_map(maps[-1][0], B, *size[-1]))
        top = laterals[-1]
        # top-down path, summed in float32 (evp_add_f32)
        f32 = [l if l.dtype == torch.float32 else ops.MapCopyFn.apply(l, torch.float32, None) for l in laterals]
        for i in range(n - 1, 0, -1):
            f32[i - 1] = ops.AddFn.apply(f32[i - 1], ops.resize_map(f32[i], B, *size[i], *size[i - 1], self.sample_mode))
        H0, W0 = size[0]
        buf = _concat_buffer(B * H0 * W0, n * ch, top.device)
        parts = []
        for i in range(n - 1):
            if size[i] == size[0]:
                parts.append(self.fpn_convs[i].on_map(f32[i], B, H0, W0, out=(buf, i * ch)))
            else:
                o = self.fpn_convs[i].on_map(f32[i], B, *size[i])
                parts.append(ops.resize_map(o, B, *size[i], H0, W0, self.sample_mode, (buf, i * ch)))
        parts.append(ops.resize_map(top, B, *size[-1], H0, W0, self.sample_mode, (buf, (n - 1) * ch)))
        feats = self.fpn_bottleneck.on_map(ops.CatFn.apply((buf,), *parts), B, H0, W0)
        return feats, B, H0, W0


class FCNHead(BaseDecodeHead):
    """FCN head: num_convs ConvModules on inputs[in_index], optionally concatenated with that input and fused by conv_cat."""

    def __init__(self, num_convs=2, kernel_size=3, concat_input=True, dilation=1, **kwargs):
        super().__init__(**kwargs)
        if dilation != 1:
            raise NotImplementedError("FCNHead: dilation 1 only")
        if num_convs < 1:
            raise ValueError("FCNHead: num_convs >= 1")
        self.concat_input = concat_input
        pad = kernel_size // 2
        convs = [ConvModule(self.in_channels, self.channels, kernel_size=kernel_size, padding=pad)]
        for _ in range(num_convs - 1):
            convs.append(ConvModule(self.channels, self.channels, kernel_size=kernel_size, padding=pad))
        self.convs = nn.Sequential(*convs)
        if concat_input:
            self.conv_cat = ConvModule(self.in_channels + self.channels, self.channels, kernel_size=kernel_size, padding=pad)

    def _forward_feature_map(self, inputs):
        m, B, H, W = to_map(inputs[self.in_index])
        buf = _concat_buffer(B * H * W, self.in_channels + self.channels, m.device) if self.concat_input else None
        feats = m
        for i, conv in enumerate(self.convs):
            last = i == len(self.convs) - 1
            feats = conv.on_map(feats, B, H, W, out=(buf, self.in_channels) if (last and buf is not None) else None)
        if self.concat_input:
            x = ops.MapCopyFn.apply(m, buf.dtype, (buf, 0))
            feats = self.conv_cat.on_map(ops.CatFn.apply((buf,), x, feats), B, H, W)
        return feats, B, H, W


def _uper(args, in_channels, **kwargs):
    return UPerHead(args=args, in_channels=in_channels, channels=384, in_index=[0, 1, 2, 3], pool_scales=(1, 2, 3, 6), **kwargs)


def _fcn(args, in_channels, **kwargs):
    return FCNHead(args=args, in_channels=in_channels, channels=256, in_index=2, num_convs=1, kernel_size=3, concat_input=False, **kwargs)


def finetune_decode_head_extend_small(args, **kwargs):
    return _uper(args, [128, 256, 384, 384], **kwargs)


def finetune_decode_head_extend_small_swin(args, **kwargs):
    return _uper(args, [96, 192, 384, 768], **kwargs)


def finetune_decode_head_extend_base(args, **kwargs):
    return _uper(args, [256, 384, 768, 768], **kwargs)


def finetune_decode_head_small(args, **kwargs):
    return _uper(args, [384, 384, 384, 384], **kwargs)


def finetune_decode_head_base(args, **kwargs):
    return _uper(args, [768, 768, 768, 768], **kwargs)


def finetune_auxiliary_head_small(args, **kwargs):
    return _fcn(args, 384, **kwargs)


def finetune_auxiliary_head_base(args, **kwargs):
    return _fcn(args, 768, **kwargs)


def finetune_auxiliary_head_small_swin(args, **kwargs):
    return _fcn(args, 384, **kwargs)
