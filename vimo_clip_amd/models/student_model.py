"""MoCLIP student on libvmc — drop-in for the reference's models/student_model.py.

Same constructor / forward signatures, attribute names (``device, preprocess, visual_encoder,
residual_mlp.{fc1,fc2,alpha}, classification_head.{0,2}``) and ``state_dict`` keys as
``FlowStudentModel`` (models/student_model.py:38-98), so reference checkpoints (keys optionally
prefixed ``module.`` by DataParallel, train.py:167) load with ``strict=True``.

Differences that are deliberate and documented:
  * there are no pretrained weights offline: ``clip.load(name)`` (:44) is replaced by building the
    named geometry with OpenAI-clip initialisation; load a checkpoint with ``load_state_dict``;
  * the per-frame CPU loop ``to_pil_image -> CLIP preprocess`` (:77-78) runs as HIP kernels: Pillow-exact
    bicubic resize + centre crop (preprocess.py) when the frames are not already 224x224, then normalisation
    fused with patch extraction; the float->PIL wrap-around (v -> (256 - v) mod 256) is
    reproduced bit-exactly for u8 / integer-valued inputs, and floating-point input goes through to_pil_image's own
    ``mul(255).byte()`` (ops.unit_f32_to_u8), which covers the MammalNet dataset's [0,1] frames as well.
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from .. import autograd_ops as ag
from .. import ops
from ..autograd_vit import vit_forward_train
from ..clip_vit import VisionTransformer, _Lin
from ..oracle_free_constants import CLIP_MEAN, CLIP_STD


class _Preprocess:
    """Stand-in for the torchvision ``Compose`` that ``clip.load`` returns (used as ``model.preprocess`` and
    ``model.preprocess.transforms`` by inference.py:90 / student_model.py:77).  The transform list is
    descriptive; the arithmetic runs inside vmc_preprocess_patches_u8."""

    def __init__(self, n_px: int):
        self.n_px = n_px
        self.transforms = [("Resize", n_px, "bicubic"), ("CenterCrop", n_px), ("ToTensor",), ("Normalize", CLIP_MEAN, CLIP_STD)]

    def __repr__(self):
        return f"CLIPPreprocess(n_px={self.n_px}, mean={CLIP_MEAN}, std={CLIP_STD})"


def _init_linear(lin: _Lin):
    nn.init.kaiming_uniform_(lin.weight, a=math.sqrt(5))
    bound = 1 / math.sqrt(lin.weight.shape[1])
    nn.init.uniform_(lin.bias, -bound, bound)


class ResidualMLP(nn.Module):
    """models/student_model.py:8-35: x + alpha * fc2(GELU(fc1(x))), fc2 zero-initialised."""

    def __init__(self, embed_dim, alpha=0.1, compute_dtype=torch.bfloat16):
        super().__init__()
        self.fc1 = _Lin(embed_dim, embed_dim)
        self.fc2 = _Lin(embed_dim, embed_dim)
        self.alpha = alpha
        self.compute_dtype = compute_dtype
        _init_linear(self.fc1)
        nn.init.zeros_(self.fc2.weight)
        nn.init.zeros_(self.fc2.bias)

    def forward(self, x):
        shape = x.shape
        x2 = x.reshape(-1, shape[-1]).contiguous()
        xa, xb = ag.fork(x2, self.compute_dtype)
        h = ag.linear(ag.cast(xa, self.compute_dtype), self.fc1.weight, self.fc1.bias, act=ops.ACT_GELU_ERF)
        m = ag.linear(h, self.fc2.weight, self.fc2.bias, out_f32=True)
        return ag.AddFn.apply(xb, m, self.alpha).view(shape)


class FlowStudentModel(nn.Module):
    def __init__(self, clip_model_name="ViT-B/32", device="cuda", num_classes=140, alpha=0.1,
                 compute_dtype=torch.bfloat16, residual_dtype=torch.float32,
                 lora_rank=0, lora_alpha=None, lora_targets=("attn",), patch_dropout=0.0, patch_dropout_seed=0,
                 drop_path=0.0, drop_path_seed=0, recompute="none"):
        """recompute: "none" or "block" (VisionTransformer.recompute: the training forward keeps one stream per block and
        recomputes the block in the backward pass; same results, a fraction of the activation memory).
        lora_rank > 0: the tower is frozen and rank-r adapters on the `lora_targets` linears of every block are trained with the two
        heads (lora.add_lora; alpha defaults to 2 rank).  0: no adapters, the model and its ``state_dict`` are what they always were.
        patch_dropout: 0 <= p < 1; in train() mode with gradients every frame keeps its class token and max(1, int(g^2 (1 - p)))
        randomly drawn patch tokens (VisionTransformer.patch_dropout), evaluation sees every token.  0: nothing is dropped.
        drop_path: 0 <= p < 1; stochastic depth per frame in train() mode with gradients: block l of L runs on max(1, int(F (1 - p l /
        (L - 1)))) randomly drawn frames of the forward (VisionTransformer.drop_path), evaluation runs every block on every frame.
        0: nothing is dropped."""
        super().__init__()
        if not 0.0 <= float(patch_dropout) < 1.0:
            raise ValueError(f"patch_dropout must satisfy 0 <= p < 1, got {patch_dropout}")
        if not 0.0 <= float(drop_path) < 1.0:
            raise ValueError(f"drop_path must satisfy 0 <= p < 1, got {drop_path}")
        if lora_rank and recompute != "none":
            raise ValueError("LoRA adapters are not supported together with recompute='block'")
        self.device = device
        self.compute_dtype = compute_dtype
        self.visual_encoder = VisionTransformer.from_name(clip_model_name, compute_dtype=compute_dtype,
                                                          residual_dtype=residual_dtype)
        self.visual_encoder.recompute = recompute
        self.visual_encoder.patch_dropout = float(patch_dropout)
        self.visual_encoder.patch_dropout_seed = int(patch_dropout_seed)
        self.visual_encoder.drop_path = float(drop_path)
        self.visual_encoder.drop_path_seed = int(drop_path_seed)
        self.preprocess = _Preprocess(self.visual_encoder.input_resolution)
        embed_dim = self.visual_encoder.output_dim
        self.residual_mlp = ResidualMLP(embed_dim, alpha=alpha, compute_dtype=compute_dtype)
        # nn.Sequential(Linear, ReLU, Linear): indices 0 and 2 carry parameters, as in the reference (:55-59)
        self.classification_head = nn.Sequential(_Lin(embed_dim, embed_dim // 2), nn.Identity(), _Lin(embed_dim // 2, num_classes))
        _init_linear(self.classification_head[0])
        _init_linear(self.classification_head[2])
        self.to(device)
        if lora_rank:
            from ..lora import add_lora
            add_lora(self.visual_encoder, lora_rank, alpha=lora_alpha, targets=lora_targets)

    def _frames_u8(self, flow_videos, unit_u8=False):
        """[B,T,C,H,W] -> (u8 frames [B*T,C,H,W] on the device, wrap_quirk): the pixels ``to_pil_image(frame)`` holds (:78), or the
        pixels whose wrap v -> (256 - v) mod 256 gives them."""
        B, T, C, H, W = flow_videos.shape
        fr = flow_videos.reshape(B * T, C, H, W)      # any H x W: Resize(R, BICUBIC) + CenterCrop(R) run PIL-exact on the GPU
        if fr.dtype == torch.uint8:
            # u8 stands for the integer-valued floats the AK datasets hand over: the reference casts to float and to_pil_image
            # multiplies by 255 and wraps to u8 (:74,:78).  unit_u8: already the PIL pixels (ops.resize_bilinear_u8(as_u8=True))
            return fr.to(self.device), not unit_u8
        if fr.is_floating_point():
            # to_pil_image itself, pic.mul(255).byte(): [0,1] floats (dataset_frame_diff_mn.py) become their pixels, integer-valued
            # floats 0..255 the wrapped pixels, the same bytes the u8 route makes of them
            return ops.unit_f32_to_u8(fr.to(self.device).float()), False
        return fr.to(torch.uint8).to(self.device), True

    def forward(self, flow_videos, *, unit_u8=False, patch_keep=None, drop_path_keep=None):
        """flow_videos [B,T,3,H,W] -> (embeddings [B,T,E], embeddings_for_distillation [B,T,E], logits [B,C]).
        unit_u8: u8 input is taken as pixels already quantised the way to_pil_image quantises [0,1] floats (no wrap).
        patch_keep: int32 [B*T, Kp] device tensor of ascending patch ids, the tokens each frame keeps (training forward only;
        None: drawn when ``patch_dropout`` > 0, in train() mode with gradients).
        drop_path_keep: one entry per residual block, None or an int32 device tensor [K_l] of ascending frame ids, the frames the block
        runs on (training forward only; None: drawn when ``drop_path`` > 0, in train() mode with gradients)."""
        B, T = flow_videos.shape[:2]
        frames, wrap = self._frames_u8(flow_videos, unit_u8)
        train = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        # live adapters: the no-grad forward runs the same launches as the training forward (concat + GEMM), so that validation
        # during training sees them; lora.merge_lora puts the model back on encode_frames_u8
        if patch_keep is not None and not train:
            raise ValueError("patch_keep needs the training forward (gradients enabled and trainable parameters)")
        if drop_path_keep is not None and not train:
            raise ValueError("drop_path_keep needs the training forward (gradients enabled and trainable parameters)")
        if train or getattr(self.visual_encoder, "lora", None) is not None:
            emb = vit_forward_train(self.visual_encoder, frames, wrap_quirk=wrap, keep=patch_keep, drop_keep=drop_path_keep)   # [B*T, E] f32
        else:
            emb = self.visual_encoder.encode_frames_u8(frames, wrap_quirk=wrap)
        return self._heads(emb, train, B, T)

    def _heads(self, emb, train, B, T):
        """Frame embeddings [B*T, E] -> the three outputs of forward (residual MLP, mean pool, classification head)."""
        if train:
            e_out, e_mlp, e_pool = _fork3(emb, self.compute_dtype)
        else:
            e_out = e_mlp = e_pool = emb
        E = emb.shape[-1]
        emb_distill = self.residual_mlp(e_mlp.view(B, T, E))
        pooled = ag.MeanPoolFn.apply(e_pool, B, T, self.compute_dtype, False)             # [B,E] 16-bit
        h = ag.linear(pooled, self.classification_head[0].weight, self.classification_head[0].bias, act=ops.ACT_RELU)
        logits = ag.linear(h, self.classification_head[2].weight, self.classification_head[2].bias, out_f32=True)
        return e_out.view(B, T, E), emb_distill, logits

    def forward_from_rgb(self, rgb_videos, prev=None):
        """rgb_videos [B,T,3,H,W] u8 -> (embeddings [B,T-1,E], embeddings_for_distillation [B,T-1,E], logits [B,C]): the motion
        frames |gray(f[t+1]) - gray(f[t])| are computed on the device (ops.frame_diff_gray: the arithmetic of the reference's
        utils/generate_frame_diff_video.py before its lossy encode) and fed to the student, so T teacher frames pair with T-1 motion
        frames (train.py:98).  Differences are taken inside a clip, never across clips.  ``prev`` [B,3,H,W] u8: one frame per clip
        that precedes it (a clip continued from an earlier chunk); every clip then yields T motion frames.
        Without gradients the grey plane goes through resize, crop and patch extraction once (encode_gray_u8); with gradients the
        three-channel differences are materialised and ``forward`` runs unchanged.  Same result either way."""
        if rgb_videos.dim() != 5 or rgb_videos.shape[2] != 3 or rgb_videos.dtype != torch.uint8:
            raise ValueError("rgb_videos must be u8 [B,T,3,H,W]")
        B, T, _, H, W = rgb_videos.shape
        n = T - 1 + (prev is not None)
        if n <= 0:
            raise ValueError("forward_from_rgb needs two frames per clip (or one and `prev`)")
        rgb = rgb_videos.to(self.device)
        prev = prev.to(self.device) if prev is not None else None
        train = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        train = train or getattr(self.visual_encoder, "lora", None) is not None      # live adapters: through forward, as in training
        ch = 3 if train else 1
        diff = torch.empty((B, n, ch, H, W), dtype=torch.uint8, device=rgb.device)
        for b in range(B):
            ops.frame_diff_gray(rgb[b], prev[b] if prev is not None else None, channels=ch, out=diff[b])
        if train:
            return self.forward(diff)
        emb = self.visual_encoder.encode_gray_u8(diff.view(B * n, 1, H, W), wrap_quirk=True)
        return self._heads(emb, False, B, n)


def _fork3(x, dt16):
    a, rest = ag.fork(x, dt16)
    b, c = ag.fork(rest, dt16)
    return a, b, c


FrameDiffStudentModel = FlowStudentModel   # models/student_model_frame_diff.py: identical arithmetic, renamed inputs
