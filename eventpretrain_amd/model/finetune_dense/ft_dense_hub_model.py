"""Dense-prediction fine-tuning hub (reference model/finetune_dense/ft_dense_hub_model.py): plain ViT backbone (its four `out_embs`
token maps) -> UPerNet decode head + FCN auxiliary head. Same constructor, factories, forward return tuple and state-dict keys
(`backbone.*`, `decode_head.*`, `auxiliary_head.*`). phase finetune_semseg: out_channels = args.num_classes; finetune_flow: 2.

ViT-Base with finetune_flow: the reference names `finetune_flow_decode_head_base` / `finetune_flow_auxiliary_head_base`, which its
decoder file does not define; the base heads with out_channels=2 are used, as its ConvViT-Base branch does.
ConvViT / Swin: their backbones here have no multi-scale `out_embs` yet and refuse the dense phases; the comparison baselines are out
of scope as in FtClsHubModel."""
import torch.nn as nn

from ..backbone import convvit, swin, vit
from ..backbone.vit import init_linear_and_norm
from . import ft_dense_decoder


class FtDenseHubModel(nn.Module):
    def __init__(self, args):
        super().__init__()
        self.args = args
        self.backbone_type = args.backbone_type
        common = dict(args=args, num_bins=args.num_bins, drop_rate=args.drop_rate, attn_drop_rate=args.attn_drop_rate,
                      drop_path_rate=args.drop_path_rate)
        if args.phase == "finetune_semseg":
            out_channels = args.num_classes
        elif args.phase == "finetune_flow":
            out_channels = 2
        else:
            raise ValueError(args.phase)
        if args.backbone_type == "vit":
            if args.model_size not in ("small", "base"):
                raise ValueError(args.model_size)
            self.backbone = vit.__dict__["vit_%s_patch16" % args.model_size](**common)
            self.decode_head = ft_dense_decoder.__dict__["finetune_decode_head_" + args.model_size](args, out_channels=out_channels)
            self.auxiliary_head = ft_dense_decoder.__dict__["finetune_auxiliary_head_" + args.model_size](args, out_channels=out_channels)
        elif args.backbone_type == "convvit":
            factory = {"small": "convvit_small_patch16", "base": "convvit_base_patch16"}
            if args.model_size not in factory:
                raise ValueError(args.model_size)
            self.backbone = convvit.__dict__[factory[args.model_size]](**common)       # raises NotImplementedError: no out_embs yet
        elif args.backbone_type == "swin":
            self.backbone = swin.__dict__["swin_tiny_window7"](**common)                # raises NotImplementedError: no out_embs yet
        elif args.backbone_type in ("vit_ecdp", "convvit_ecdp", "vit_mem", "swin_ecddp"):
            raise NotImplementedError("%s is one of the reference's comparison baselines (out of scope)" % args.backbone_type)
        else:
            raise ValueError(args.backbone_type)
        if not hasattr(self, "decode_head"):
            raise NotImplementedError("dense heads are wired for the plain ViT backbones only (%s)" % args.backbone_type)
        self.apply(init_linear_and_norm)          # nn.Linear / nn.LayerNorm only: the heads keep torch's Conv2d / BatchNorm2d defaults

    def forward(self, x):
        emb_l1, emb_l2, emb_h, out_embs, attn = self.backbone(x)
        decode_predict = self.decode_head(out_embs)
        aux_predict = self.auxiliary_head(out_embs)
        return emb_l1, emb_l2, emb_h, out_embs, attn, decode_predict, aux_predict


def finetune_dense_hub_model_small_patch16(args):
    return FtDenseHubModel(args=args)


def finetune_dense_hub_model_base_patch16(args):
    return FtDenseHubModel(args=args)
