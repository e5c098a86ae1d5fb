"""GPU: FlowStudentModel on the 336-px towers (577 tokens).  The training forward takes SelfAttnPackedFn's ViT route past 288 tokens
(attention_vit_long.hip, lse kept) and the backward the tiled kernels of attention_long.hip.  Bounds as in test_gpu_models.py."""
import pytest
import torch

from oracle import student as ostudent
from vimo_clip_amd import synth

pytestmark = pytest.mark.gpu
TINY = "ViT-tiny/14@336px"


def _student(name, seed, dtype):
    from vimo_clip_amd.models import FlowStudentModel
    m = FlowStudentModel(name, device="cuda", num_classes=140, alpha=0.1, compute_dtype=dtype)
    sd = synth.student_state_dict(name, seed)
    m.load_state_dict(sd, strict=True)
    return m, sd


def test_tiny336_student_forward_vs_oracle():
    m, sd = _student(TINY, 23, torch.float16)
    m.eval()
    vids = synth.randint_u8(23, "vids", (2, 3, 3, 336, 336))
    with torch.no_grad():
        out = m(vids.cuda())
    ref = ostudent.student_forward(sd, vids, 2, alpha=0.1, wrap_quirk=True)
    for got, want in zip(out, ref):
        err = (got.float().cpu() - want).abs().max().item()
        assert err <= 2e-3 * max(1.0, want.abs().max().item()), err


def test_tiny336_student_train_step_vs_oracle_autograd():
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    B, T = 2, 3
    m, sd = _student(TINY, 29, torch.bfloat16)
    m.train()
    vids = synth.randint_u8(29, "vids", (B, T, 3, 336, 336))
    teacher = synth.normal(29, "teacher", (B, T + 1, 96))
    labels = synth.multi_hot_labels(29, "labels", B, 140)
    emb, emb_d, logits = m(vids.cuda())
    loss = distillation_loss(emb_d, teacher.cuda()[:, :-1, :], mode="cosine") + classification_loss(logits, labels.cuda(), positive_weight=9)
    loss.backward()
    sdo = {k: v.clone().requires_grad_(True) for k, v in sd.items()}
    _, oe_d, ol = ostudent.student_forward(sdo, vids, 2, alpha=0.1, wrap_quirk=True)
    oloss = ostudent.distillation_loss(oe_d, teacher[:, :-1, :], "cosine") + ostudent.classification_loss(ol, labels, 9)
    oloss.backward()
    assert abs(loss.item() - oloss.item()) <= 1e-2 * abs(oloss.item())
    worst = 0.0
    for k, p in m.named_parameters():
        ref = sdo[k].grad
        rel = (p.grad.cpu() - ref).abs().max().item() / (ref.abs().max().item() + 1e-12)
        worst = max(worst, rel)
        assert rel <= 8e-2, (k, rel)
    print(f"tiny-336 student step: loss {loss.item():.5f} vs {oloss.item():.5f}; worst grad rel-to-max err {worst:.3e}")


def test_vit_l14_336_student_step_is_finite():
    from vimo_clip_amd.losses import classification_loss, distillation_loss
    name = "ViT-L/14@336px"
    m, _ = _student(name, 2, torch.bfloat16)
    assert m.preprocess.n_px == 336
    m.train()
    vids = synth.randint_u8(2, "vids", (1, 3, 3, 336, 336))
    teacher = synth.normal(2, "teacher", (1, 4, 768))
    labels = synth.multi_hot_labels(2, "labels", 1, 140)
    emb, emb_d, logits = m(vids.cuda())
    assert emb.shape[-1] == 768 and emb_d.shape[-1] == 768
    loss = distillation_loss(emb_d, teacher.cuda()[:, :-1, :], mode="cosine") + classification_loss(logits, labels.cuda(), positive_weight=9)
    loss.backward()
    assert torch.isfinite(loss).item()
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all().item(), k
