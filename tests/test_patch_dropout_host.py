"""CPU: the keep-set sampler's reference (tests/patch_dropout_ref.py, built on attention_refs.hash32) and the host side of patch
dropout: the Kp rule, argument validation before anything touches a device, the --patch_dropout flags, and the byte model at N'."""
import numpy as np
import pytest
import torch

import patch_dropout_ref as PR


# ---------------------------------------------------------------------------------------------- the sampler's reference
@pytest.mark.parametrize("seed,F,G,Kp", [(1, 3, 16, 4), (0x1234567, 3, 49, 24), (99, 2, 576, 144), (5, 2, 16, 1), ((1 << 63) - 1, 4, 1024, 512)])
def test_reference_rows_are_sorted_unique_and_in_range(seed, F, G, Kp):
    keep = PR.keep_sample(seed, F, G, Kp)
    assert keep.shape == (F, Kp) and keep.dtype == np.int32
    assert keep.min() >= 0 and keep.max() < G
    assert (np.diff(keep, axis=1) > 0).all()                       # strictly ascending: sorted and unique


def test_reference_keeps_the_smallest_keys():
    """Every kept patch is in front of every dropped one in the order (key, id)."""
    from attention_refs import hash32
    seed, F, G, Kp = 77, 3, 49, 24
    keep = PR.keep_sample(seed, F, G, Kp)
    for f in range(F):
        key = hash32(seed, np.uint64(f * G) + np.arange(G, dtype=np.uint64)).astype(np.int64)
        rank = key * G + np.arange(G)                              # (key, id) as one integer
        kept = np.zeros(G, dtype=bool)
        kept[keep[f]] = True
        assert rank[kept].max() < rank[~kept].min()


def test_reference_identity_and_difference():
    assert (PR.keep_sample(3, 2, 16, 16) == np.arange(16)[None, :]).all()           # Kp = G: every patch, in order
    a = PR.keep_sample(3, 4, 49, 24)
    assert len({tuple(r) for r in a}) == 4                                           # frames draw different sets
    b = PR.keep_sample(4, 4, 49, 24)
    assert all(tuple(x) != tuple(y) for x, y in zip(a, b))                           # ... and so do seeds
    assert (PR.keep_sample(3, 4, 49, 24) == a).all()                                 # a pure function of its arguments


def test_reference_inclusion_is_uniform_within_the_binomial_tail():
    """2 000 fixed seeds, one frame, G = 16, Kp = 4: under a uniform sampler each patch's inclusion count is Binomial(2000, 1/4).
    The bound is the smallest deviation that ANY of the 16 counts reaches with probability at most 1e-6 (union bound over the exact
    binomial tail) -- nothing read off the sampler."""
    n, G, Kp = 2000, 16, 4
    counts = np.zeros(G, dtype=np.int64)
    for seed in range(1, n + 1):
        counts[PR.keep_sample(seed * 0x9E3779B1, 1, G, Kp)[0]] += 1
    assert counts.sum() == n * Kp
    sd = (n * (Kp / G) * (1 - Kp / G)) ** 0.5
    worst = np.abs(counts - n * Kp / G).max()
    bound = PR.inclusion_deviation_bound(n, G, Kp)
    print(f"inclusion counts {counts.tolist()}: largest deviation {worst:.0f} = {worst / sd:.2f} sd; bound {bound} = {bound / sd:.2f} sd")
    assert 4.0 * sd < bound < 7.0 * sd                            # the bound itself is where a 1e-6 / 32 normal tail puts it
    assert worst < bound


def test_binomial_tail_helper():
    assert PR.binomial_two_sided_tail(10, 0.5, 0) == pytest.approx(1.0)
    assert PR.binomial_two_sided_tail(10, 0.5, 5) == pytest.approx(2 / 1024)        # X = 0 or 10
    assert PR.binomial_two_sided_tail(4, 0.25, 2) == pytest.approx(4 * 0.25 ** 3 * 0.75 + 0.25 ** 4)      # X = 3 or 4


def test_reference_assembly_and_its_backward():
    """The restatements agree with a direct loop on a hand-sized case."""
    F, G, Kp, D = 2, 4, 2, 4
    keep = np.array([[0, 3], [1, 2]], dtype=np.int32)
    xp = torch.arange(F * Kp * D, dtype=torch.float32).view(F * Kp, D).to(torch.bfloat16)
    cls, pos = torch.full((D,), 0.5), torch.arange((G + 1) * D, dtype=torch.float32).view(G + 1, D) * 0.25
    x = PR.assemble_keep(xp, cls, pos, keep, torch.float32).view(F, Kp + 1, D)
    assert torch.equal(x[0, 0], cls + pos[0]) and torch.equal(x[1, 2], xp[3].float() + pos[3])
    dxp, dpos, mag = PR.assemble_keep_bwd(x.view(-1, D), keep, G, torch.bfloat16)
    assert torch.equal(dxp, x[:, 1:].reshape(-1, D).to(torch.bfloat16))
    assert np.array_equal(dpos[0], (x[0, 0] + x[1, 0]).double().numpy()) and np.array_equal(dpos[4], x[0, 2].double().numpy())
    assert np.array_equal(dpos[2], x[1, 1].double().numpy()) and (mag >= np.abs(dpos)).all()
    assert np.array_equal(PR.gather_rows(np.arange(8).reshape(8, 1), keep, G)[:, 0], [0, 3, 5, 6])


# ---------------------------------------------------------------------------------------------- host logic
def test_keep_count_rule():
    from vimo_clip_amd import ops
    for G, p, want in ((16, 0.5, 8), (16, 0.75, 4), (49, 0.5, 24), (49, 0.75, 12), (576, 0.75, 144), (576, 0.5, 288), (256, 0.9, 25), (4, 0.9, 1),
                       (16, 0.99, 1), (16, 0.0, 16)):
        assert ops.patch_keep_count(G, p) == want == PR.keep_count(G, p), (G, p)


def _student(**kw):
    from vimo_clip_amd.models.student_model import FlowStudentModel
    torch.manual_seed(0)
    return FlowStudentModel("ViT-tiny/14", device="cpu", num_classes=12, **kw)


def test_flags_and_their_defaults():
    from vimo_clip_amd.clip_vit import VisionTransformer
    v = VisionTransformer.from_name("ViT-tiny/32")
    assert v.patch_dropout == 0.0 and v.patch_dropout_seed == 0 and v.patch_dropout_seed_address is None
    m = _student()
    assert m.visual_encoder.patch_dropout == 0.0
    m = _student(patch_dropout=0.5, patch_dropout_seed=11)
    assert m.visual_encoder.patch_dropout == 0.5 and m.visual_encoder.patch_dropout_seed == 11
    assert set(m.state_dict()) == set(_student().state_dict())                       # a flag, not a parameter
    for bad in (1.0, -0.1, 1.5):
        with pytest.raises(ValueError, match="patch_dropout"):
            _student(patch_dropout=bad)


def test_nothing_is_drawn_without_training_or_gradients():
    """patch_keep_for returns None -- before any device call: these towers live on the CPU -- unless p > 0, train() and grad."""
    from vimo_clip_amd.autograd_vit import patch_keep_for
    from vimo_clip_amd.clip_vit import VisionTransformer
    v = VisionTransformer.from_name("ViT-tiny/32").train()
    assert patch_keep_for(v, 4, "cpu") is None                                        # p = 0
    v.patch_dropout = 0.5
    with torch.no_grad():
        assert patch_keep_for(v, 4, "cpu") is None
    assert patch_keep_for(v.eval(), 4, "cpu") is None
    assert getattr(v, "_patch_dropout_calls", 0) == 0                                 # none of them consumed a draw
    v.train().patch_dropout = 1.0
    with pytest.raises(ValueError, match="patch_dropout"):
        patch_keep_for(v, 4, "cpu")


def test_keep_tensor_validation_precedes_the_device():
    from vimo_clip_amd import ops
    src = torch.zeros((2 * 16, 64), dtype=torch.bfloat16)
    with pytest.raises(ValueError, match="int32"):
        ops.gather_rows16(src, torch.zeros((2, 4), dtype=torch.int64), 16)
    with pytest.raises(ValueError, match="F = 2"):
        ops.gather_rows16(src, torch.zeros((3, 4), dtype=torch.int32), 16)
    with pytest.raises(ValueError, match="patches per frame"):
        ops.gather_rows16(src, torch.zeros((2, 17), dtype=torch.int32), 16)
    with pytest.raises(ValueError, match="16-bit"):
        ops.gather_rows16(src.float(), torch.zeros((2, 4), dtype=torch.int32), 16)
    with pytest.raises(RuntimeError, match="no CPU path"):                             # valid arguments: there is no fallback
        ops.gather_rows16(src, torch.zeros((2, 4), dtype=torch.int32), 16)
    m = _student()
    with pytest.raises(ValueError, match="patch_keep"):
        with torch.no_grad():
            m(torch.zeros((1, 2, 3, 56, 56), dtype=torch.uint8), patch_keep=torch.zeros((2, 4), dtype=torch.int32))


def test_patch_dropout_flag_parsing():
    from vimo_clip_amd import train, train_frame_diff_mn
    a = train.build_parser().parse_args([])
    assert not hasattr(a, "patch_dropout") and train.patch_dropout_kwargs(a) == {}    # a run without it: the namespace it always had
    a = train.build_parser().parse_args(["--patch_dropout", "0.5"])
    assert a.patch_dropout == 0.5
    assert train.patch_dropout_kwargs(a) == {"patch_dropout": 0.5, "patch_dropout_seed": train.PATCH_DROPOUT_SEED}
    assert train.patch_dropout_kwargs(a, rank=3)["patch_dropout_seed"] == train.PATCH_DROPOUT_SEED + 3      # a stream per rank
    assert train.patch_dropout_kwargs(train.build_parser().parse_args(["--patch_dropout", "0"])) == {}
    for bad in ("1", "1.0", "-0.25", "half"):
        with pytest.raises(SystemExit):
            train.build_parser().parse_args(["--patch_dropout", bad])
    need = ["--train_hdf5_path", "a", "--val_hdf5_path", "b", "--frame_diff_videos_dir", "c"]
    q = train_frame_diff_mn.build_parser()
    assert q.parse_args(need).patch_dropout == 0.0 and train.patch_dropout_kwargs(q.parse_args(need)) == {}
    assert q.parse_args(need + ["--patch_dropout", "0.75"]).patch_dropout == 0.75
    assert q.parse_args(need + ["--patch-dropout", "0.25"]).patch_dropout == 0.25
    m = _student(**train.patch_dropout_kwargs(a, rank=1))
    assert m.visual_encoder.patch_dropout == 0.5 and m.visual_encoder.patch_dropout_seed == train.PATCH_DROPOUT_SEED + 1


def test_saved_activation_bytes_at_the_kept_token_count():
    from vimo_clip_amd.autograd_vit import saved_activation_bytes as sab
    name, (R, p, D, L, H, _E) = "ViT-B/32", (224, 32, 768, 12, 12, 512)
    assert sab(name, 3, tokens=50) == sab(name, 3) and sab(name, 3, "block", tokens=50) == sab(name, 3, "block")
    # 25 rows per frame (Kp = 24 of 49): per row and block 36 D + 4 H + 16; the last block's MLP half on the class row only
    row_attn, row_mlp = 14 * D + 4 * H + 8, 22 * D + 8
    assert sab(name, 1, cls_only=False, tokens=25) == L * 25 * (row_attn + row_mlp)
    assert sab(name, 1, tokens=25) == (L - 1) * 25 * (row_attn + row_mlp) + 25 * row_attn + (2 * D + row_mlp)
    assert sab(name, 2, "block", tokens=25) == 2 * L * 25 * 4 * D
    assert sab(name, 1, cls_only=False, tokens=25) * 2 == sab(name, 1, cls_only=False)          # rows are what every term scales with
    for bad in (1, 51, 0):
        with pytest.raises(ValueError, match="tokens"):
            sab(name, 1, tokens=bad)
