"""On-device augmentation of triplets (staging.hip, mauv/augment.py).

* The draw is bit-equal to oracle/philox_ref (integer words, fp32 uniforms rounded step by
  step) in numpy.
* A move is pure data movement, so every augmented entry is held ``torch.equal`` to the
  existing un-augmented entry on the device followed by the recipe
  ``bit1: flip(-2); bit0: flip(-1); bit2: transpose(-2, -1)`` — explicit codes [0..7, 5], so
  every code appears whatever the draw gives.  Shapes: odd sizes with a W tail of 1 (13), a
  multiple of the 4-pixel vector (16), a non-square tile with flips only, one channel, B = 0.
* One un-moved case against oracle/staging_ref with the bars of test_staging_metrics_gpu.py:
  exact for ToTensor / Normalize, atol 5e-7 for the UIFM (exp may differ by one ulp between
  libm implementations; outputs in [0, 1]).
* Per-item turbidity: item b equals the existing scalar call on that item alone.
"""
import numpy as np
import pytest
import torch

from oracle import staging_ref
from oracle.philox_ref import philox4x32_10, uniforms32

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
CODES9 = [0, 1, 2, 3, 4, 5, 6, 7, 5]
FLIPS5 = [0, 1, 2, 3, 2]
AUG_LAYER = 0x41554721


def _codes(c):
    return torch.tensor(c, dtype=torch.uint8, device=DEV)


def moved(x, codes, hdim=-2):
    """The issue's recipe, item by item, on [B, ..] tensors whose H, W are dims hdim, hdim + 1
    (counted from the end)."""
    out = []
    for xb, k in zip(x, codes):
        y = xb
        if k & 2:
            y = y.flip(hdim)
        if k & 1:
            y = y.flip(hdim + 1)
        if k & 4:
            y = y.transpose(hdim, hdim + 1)
        out.append(y)
    return torch.stack(out).contiguous() if out else x.clone()


def _tiles(B, H, W, C, seed=0):
    g = torch.Generator().manual_seed(seed + B * 1000 + H * 10 + W + C)
    return torch.randint(0, 256, (B, H, W, C), generator=g, dtype=torch.uint8)


def _dmap(B, H, W, seed=1):
    g = torch.Generator().manual_seed(seed + B + H + W)
    return (torch.rand(B, 1, H, W, generator=g) * 2 + 0.05).to(DEV)


def _f32(vals):
    return torch.tensor(np.asarray(vals, dtype=np.float32), device=DEV)


# ------------------------------------------------------------------------------------ draw
def _draw_ref(seed, step, item0, B, mode, lo, hi):
    r = philox4x32_10(np.arange(item0, item0 + B, dtype=np.uint64), step, AUG_LAYER, seed)
    ops = (r[:, 0] >> np.uint32(30 if mode == 1 else 29)).astype(np.uint8)
    u = uniforms32(r[:, 1]).astype(np.float32)
    lo, hi = np.float32(lo), np.float32(hi)
    span = np.float32(hi - lo)
    turb = (lo + (span * u).astype(np.float32)).astype(np.float32)
    return ops, turb


def _draw(seed, step, item0, B, mode, lo=0.3, hi=1.5, turb=True):
    from mauv import ops
    o = torch.full((B,), 255, dtype=torch.uint8, device=DEV)
    t = torch.full((B,), -1.0, device=DEV) if turb else None
    ops.augment_draw(seed, step, item0, mode, lo, hi, o, t)
    return o, t


@pytest.mark.parametrize("seed,step", [(2024, 0), (2024, 1), (7, 3)])
@pytest.mark.parametrize("mode", [1, 2])
def test_draw_bit_equal_to_philox_oracle(seed, step, mode):
    ops_r, turb_r = _draw_ref(seed, step, 0, 64, mode, 0.3, 1.5)
    assert set(ops_r.tolist()) == set(range(4 if mode == 1 else 8))   # every code occurs
    assert turb_r.min() >= np.float32(0.3) and turb_r.max() <= np.float32(1.5)
    o, t = _draw(seed, step, 0, 64, mode)
    assert np.array_equal(o.cpu().numpy(), ops_r)
    assert np.array_equal(t.cpu().numpy().view(np.uint32), turb_r.view(np.uint32))
    # item0: two half draws are the whole one
    o0, t0 = _draw(seed, step, 0, 32, mode)
    o1, t1 = _draw(seed, step, 32, 32, mode)
    assert torch.equal(torch.cat([o0, o1]), o) and torch.equal(torch.cat([t0, t1]), t)


def test_draw_modes_and_optional_turbidity():
    o, t = _draw(2024, 5, 0, 64, 0, turb=False)
    assert t is None and not o.any().item()
    o, _ = _draw(2024, 2 ** 40 + 3, 2 ** 32 - 64, 64, 2, turb=False)   # 64-bit step, last items
    ops_r, _ = _draw_ref(2024, 2 ** 40 + 3, 2 ** 32 - 64, 64, 2, 0.3, 1.5)
    assert np.array_equal(o.cpu().numpy(), ops_r)
    o, t = _draw(3, 0, 0, 64, 2, lo=0.9, hi=0.9)
    assert torch.equal(t, torch.full((64,), np.float32(0.9).item(), device=DEV))


# -------------------------------------------------------------------------- moves, bit-exact
U8_CASES = [(9, 13, 13, 3, True, CODES9, True), (9, 16, 16, 1, False, CODES9, True),
            (5, 17, 12, 3, True, FLIPS5, False), (0, 8, 8, 3, True, [], True)]


def _uifm_host(C, turb):
    beta = np.asarray([0.8, 0.5, 0.3][:C], dtype=np.float32)
    return _f32(beta * np.float32(turb)), _f32([0.1, 0.3, 0.5][:C]), _f32(beta)


def _stage_u8_plain(tiles, mean, std, bt, binf, dist, depth):
    from mauv import ops
    from mauv._lib import lib, check
    B, H, W, C = tiles.shape
    out = torch.empty(B, C, H, W, device=DEV)
    check(lib.mauv_stage_u8(tiles.data_ptr(), B, H, W, C, ops._p(mean), ops._p(std), ops._p(bt),
                            ops._p(binf), ops._p(dist), depth, out.data_ptr(), ops.stream()))
    return out


@pytest.mark.parametrize("degrade", [False, True], ids=["plain", "uifm_map"])
@pytest.mark.parametrize("B,H,W,C,norm,codes,tr", U8_CASES,
                         ids=["9x13x13x3", "9x16x16x1", "5x17x12x3_flips", "B0"])
def test_stage_u8_aug_is_plain_then_move(B, H, W, C, norm, codes, tr, degrade):
    from mauv import ops
    from mauv.staging import OPTICAL_MEAN, OPTICAL_STD
    tiles = _tiles(B, H, W, C).to(DEV)
    mean, std = (_f32(OPTICAL_MEAN), _f32(OPTICAL_STD)) if norm else (None, None)
    bt = binf = dist = None
    if degrade:                       # a non-uniform distance map: it must move with the image
        bt, binf, _ = _uifm_host(C, 0.7)
        dist = _dmap(B, H, W)
    ref = _stage_u8_plain(tiles, mean, std, bt, binf, dist, 1.25)
    got = torch.full((B, C, H, W), float("nan"), device=DEV)
    ops.stage_u8_aug(tiles, mean, std, bt, binf, dist, 1.25, _codes(codes), None, tr, got)
    assert torch.equal(got, moved(ref, codes))
    # no codes, no turbidity: the bits of the existing entry
    got2 = torch.full((B, C, H, W), float("nan"), device=DEV)
    ops.stage_u8_aug(tiles, mean, std, bt, binf, dist, 1.25, None, None, False, got2)
    assert torch.equal(got2, ref)
    if B and not tr:                  # allow_transpose == 0: bit2 of a code is not read
        got3 = torch.empty_like(got)
        ops.stage_u8_aug(tiles, mean, std, bt, binf, dist, 1.25, _codes([k | 4 for k in codes]),
                         None, False, got3)
        assert torch.equal(got3, got)


RESIZE_CASES = [(40, 31, 16, 16, 3, CODES9, True), (16, 31, 16, 16, 1, CODES9, True),
                (31, 16, 16, 16, 3, CODES9, True), (16, 16, 16, 16, 3, CODES9, True),
                (37, 23, 12, 20, 3, FLIPS5, False)]


def _resize_aug(tiles, Ho, Wo, u8, mean, std, bt, binf, dist, depth, codes, turb, tr):
    from mauv import ops
    from mauv._lib import lib
    B, H, W, C = tiles.shape
    ws = torch.empty(max(int(lib.mauv_resize_workspace_bytes(B, H, W, C, Ho, Wo)), 1),
                     dtype=torch.uint8, device=DEV)
    o8 = torch.full((B, Ho, Wo, C), 77, dtype=torch.uint8, device=DEV) if u8 else None
    of = None if u8 else torch.full((B, C, Ho, Wo), float("nan"), device=DEV)
    ops.resize_u8_aug(tiles, Ho, Wo, ws, o8, mean, std, bt, binf, dist, depth, codes, turb, tr, of)
    return o8 if u8 else of


@pytest.mark.parametrize("H,W,Ho,Wo,C,codes,tr", RESIZE_CASES,
                         ids=["both", "horizontal", "vertical", "no_pass", "37x23_flips"])
def test_resize_u8_aug_is_plain_then_move(H, W, Ho, Wo, C, codes, tr):
    from mauv import staging
    B = len(codes)
    tiles = _tiles(B, H, W, C).to(DEV)
    k = _codes(codes)
    # 8-bit output [B, Ho, Wo, C]: H, W are dims -3, -2 of an item
    ref8 = staging.resize(tiles, (Ho, Wo))
    got8 = _resize_aug(tiles, Ho, Wo, True, None, None, None, None, None, 1.0, k, None, tr)
    assert torch.equal(got8, moved(ref8, codes, hdim=-3))
    assert torch.equal(_resize_aug(tiles, Ho, Wo, True, None, None, None, None, None, 1.0, None,
                                   None, False), ref8)
    # fused fp32 output: ToTensor only, then Normalize + UIFM over a non-uniform map (C = 3)
    reff = staging.resize_to_tensor(tiles, (Ho, Wo))
    gotf = _resize_aug(tiles, Ho, Wo, False, None, None, None, None, None, 1.0, k, None, tr)
    assert torch.equal(gotf, moved(reff, codes))
    if C == 3:
        dist = _dmap(B, Ho, Wo)
        mean, std = staging.OPTICAL_MEAN, staging.OPTICAL_STD
        reff = staging.resize_to_tensor(tiles, (Ho, Wo), mean, std, degrade=(0.7, 1.25, dist))
        bt, binf, _ = _uifm_host(3, 0.7)
        args = (tiles, Ho, Wo, False, _f32(mean), _f32(std), bt, binf, dist, 1.25)
        assert torch.equal(_resize_aug(*args, k, None, tr), moved(reff, codes))
        assert torch.equal(_resize_aug(*args, None, None, False), reff)


def _uifm_plain(x, bt, binf, dist, depth):
    from mauv import ops
    from mauv._lib import lib, check
    B, C, H, W = x.shape
    out = torch.empty_like(x)
    check(lib.mauv_uifm(x.data_ptr(), B, C, H, W, bt.data_ptr(), binf.data_ptr(), ops._p(dist),
                        depth, out.data_ptr(), ops.stream()))
    return out


@pytest.mark.parametrize("uifm", [False, True], ids=["move", "uifm_map"])
@pytest.mark.parametrize("B,C,H,W,codes,tr", [(9, 3, 13, 13, CODES9, True),
                                              (9, 1, 64, 64, CODES9, True),
                                              (5, 2, 17, 12, FLIPS5, False)],
                         ids=["9x3x13x13", "9x1x64x64", "5x2x17x12_flips"])
def test_stage_f32_aug_is_plain_then_move(B, C, H, W, codes, tr, uifm):
    from mauv import ops
    g = torch.Generator().manual_seed(B + C + H)
    x = torch.randn(B, C, H, W, generator=g).to(DEV)
    bt = binf = dist = None
    ref = x
    if uifm:
        bt, binf, _ = _uifm_host(C, 1.1)
        dist = _dmap(B, H, W)
        ref = _uifm_plain(x, bt, binf, dist, 0.8)
    got = torch.full_like(x, float("nan"))
    ops.stage_f32_aug(x, bt, binf, dist, 0.8, _codes(codes), None, tr, got)
    assert torch.equal(got, moved(ref, codes))
    got2 = torch.full_like(x, float("nan"))
    ops.stage_f32_aug(x, bt, binf, dist, 0.8, None, None, False, got2)
    assert torch.equal(got2, ref)


def test_unmoved_result_against_cpu_oracle():
    """Codes of 0 through the augmented kernel: ToTensor / Normalize exact against
    oracle/staging_ref, the per-item UIFM (one turbidity for all) within 5e-7 of it."""
    from mauv import ops
    from mauv.staging import OPTICAL_MEAN, OPTICAL_STD
    B, H, W = 3, 17, 13
    tiles = _tiles(B, H, W, 3)
    zero = _codes([0] * B)
    mean, std = _f32(OPTICAL_MEAN), _f32(OPTICAL_STD)
    got = torch.empty(B, 3, H, W, device=DEV)
    ops.stage_u8_aug(tiles.to(DEV), mean, std, None, None, None, 1.0, zero, None, False, got)
    x = staging_ref.to_tensor_normalize(tiles, OPTICAL_MEAN, OPTICAL_STD)
    assert torch.equal(got.cpu(), x)
    dist = _dmap(B, H, W)
    _, binf, beta = _uifm_host(3, 1.0)
    ops.stage_u8_aug(tiles.to(DEV), mean, std, beta, binf, dist, 1.0, zero,
                     _f32([0.7] * B), False, got)
    ref = staging_ref.simulate_underwater_degradation(x, dist.cpu(), 0.7, 1.0)
    np.testing.assert_allclose(got.cpu().numpy(), ref.numpy(), rtol=0, atol=5e-7)


# ----------------------------------------------------------------------- per-item turbidity
def test_per_item_turbidity_is_the_scalar_call_per_item():
    from mauv import ops, staging
    B, H, W = 4, 13, 13
    tiles = _tiles(B, H, W, 3).to(DEV)
    turb = [0.3, 0.77, 1.5, 1.0000001]
    tv = _f32(turb)
    mean, std = staging.OPTICAL_MEAN, staging.OPTICAL_STD
    _, binf, beta = _uifm_host(3, 1.0)
    dist = _dmap(B, H, W)
    xf = staging.to_tensor_normalize(tiles, mean, std)
    got_u8 = torch.empty(B, 3, H, W, device=DEV)
    ops.stage_u8_aug(tiles, _f32(mean), _f32(std), beta, binf, dist, 1.25, None, tv, False, got_u8)
    got_rs = _resize_aug(tiles, 16, 16, False, _f32(mean), _f32(std), beta, binf, None, 1.25, None,
                         tv, False)
    got_f = torch.empty_like(xf)
    ops.stage_f32_aug(xf, beta, binf, dist, 1.25, None, tv, False, got_f)
    for b in range(B):
        t = float(tv[b].item())
        one = slice(b, b + 1)
        assert torch.equal(got_u8[one], staging.to_tensor_normalize(
            tiles[one], mean, std, degrade=(t, 1.25, dist[one])))
        assert torch.equal(got_rs[one], staging.resize_to_tensor(
            tiles[one], (16, 16), mean, std, degrade=(t, 1.25)))
        assert torch.equal(got_f[one], staging.simulate_underwater_degradation(
            xf[one], dist[one], t, 1.25))
    # all turbidities equal: the whole batch is today's scalar call
    same = _f32([0.77] * B)
    ops.stage_u8_aug(tiles, _f32(mean), _f32(std), beta, binf, dist, 1.25, None, same, False,
                     got_u8)
    assert torch.equal(got_u8, staging.to_tensor_normalize(
        tiles, mean, std, degrade=(float(same[0].item()), 1.25, dist)))
    ops.stage_f32_aug(xf, beta, binf, dist, 1.25, None, same, False, got_f)
    assert torch.equal(got_f, staging.simulate_underwater_degradation(
        xf, dist, float(same[0].item()), 1.25))


# ----------------------------------------------------------------- round trips and autograd
def test_round_trip_and_autograd():
    from mauv import dihedral, undo_dihedral
    g = torch.Generator().manual_seed(11)
    x = torch.randn(9, 3, 13, 13, generator=g).to(DEV)
    w = torch.randn(9, 3, 13, 13, generator=g).to(DEV)
    k = _codes(CODES9)
    y = dihedral(x, k)
    assert torch.equal(y, moved(x, CODES9))
    assert torch.equal(undo_dihedral(y, k), x)
    assert torch.equal(dihedral(undo_dihedral(x, k), k), x)
    xr = x.clone().requires_grad_(True)
    (w * dihedral(xr, k)).sum().backward()
    assert torch.equal(xr.grad, undo_dihedral(w, k))
    # a non-square tile: flips only, bit2 is not read
    z = torch.randn(5, 2, 17, 12, generator=g).to(DEV)
    kf = _codes(FLIPS5)
    assert torch.equal(dihedral(z, kf), moved(z, FLIPS5))
    assert torch.equal(undo_dihedral(dihedral(z, kf), kf), z)
    with pytest.raises(ValueError, match="square"):
        dihedral(z, kf, allow_transpose=True)


@pytest.mark.parametrize("H,W,tr", [(17, 12, None), (17, 12, False), (16, 16, False)],
                         ids=["17x12", "17x12_explicit", "16x16_no_transpose"])
def test_codes_with_bit2_where_the_transpose_is_not_read(H, W, tr):
    """Every code 0..7 on a tile whose bit2 is not read (non-square, or allow_transpose=False):
    code k acts as k & 3 in the move, in its inverse and in its gradient alike."""
    from mauv import dihedral, undo_dihedral
    g = torch.Generator().manual_seed(H + W)
    x = torch.randn(8, 2, H, W, generator=g).to(DEV)
    w = torch.randn(8, 2, H, W, generator=g).to(DEV)
    codes = list(range(8))
    k = _codes(codes)
    y = dihedral(x, k, tr)
    assert torch.equal(y, moved(x, [c & 3 for c in codes]))
    assert torch.equal(undo_dihedral(y, k, tr), x)
    assert torch.equal(dihedral(undo_dihedral(x, k, tr), k, tr), x)
    xr = x.clone().requires_grad_(True)
    (w * dihedral(xr, k, tr)).sum().backward()
    assert torch.equal(xr.grad, undo_dihedral(w, k, tr))
    assert torch.equal(xr.grad, moved(w, [c & 3 for c in codes]))    # a flip undoes itself


def test_backward_is_once_differentiable():
    """A second differentiation (the incoming gradient itself requires grad) raises instead of
    cutting the graph silently: the backward is an opaque kernel call."""
    from mauv import dihedral
    x = torch.randn(2, 1, 4, 4, device=DEV, requires_grad=True)
    w = torch.randn(2, 1, 4, 4, device=DEV, requires_grad=True)
    (gx,) = torch.autograd.grad((w * dihedral(x, _codes([5, 6]))).sum(), x, create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable"):
        gx.sum().backward()


# --------------------------------------------------------------------------------- coherence
def test_triplet_gets_one_plan_and_only_the_optical_tile_is_degraded():
    from mauv import TripletAugment, dihedral, staging
    B = 9
    opt = _tiles(B, 32, 32, 3, seed=3).to(DEV)
    sss = _tiles(B, 32, 32, 1, seed=4).to(DEV)
    bathy = torch.rand(B, 3, 32, 32, generator=torch.Generator().manual_seed(5)).to(DEV)
    aug = TripletAugment("dihedral", turbidity=(0.3, 1.5), depth=1.0, seed=2024)
    o, b, s = aug(opt, bathy, sss)
    plan = aug.last_plan
    assert plan.step == 0 and aug.step == 1 and plan.ops.dtype == torch.uint8
    ops_r, turb_r = _draw_ref(2024, 0, 0, B, 2, 0.3, 1.5)
    assert np.array_equal(plan.ops.cpu().numpy(), ops_r)
    assert np.array_equal(plan.turb.cpu().numpy(), turb_r)
    assert len(set(ops_r.tolist())) > 2 and (ops_r >= 4).any()
    mean, std = staging.OPTICAL_MEAN, staging.OPTICAL_STD
    degraded = torch.cat([staging.resize_to_tensor(opt[i:i + 1], staging.TILE_SIZE, mean, std,
                                                   degrade=(float(turb_r[i]), 1.0))
                          for i in range(B)])
    assert torch.equal(o, dihedral(degraded, plan.ops))
    assert torch.equal(b, dihedral(bathy, plan.ops))
    assert torch.equal(s, dihedral(staging.stage_tile_batch(sss, False), plan.ops))
    # the same plan again gives the same tensors; the next draw is another step
    o2, b2, s2 = aug.apply(plan, opt, bathy, sss)
    assert torch.equal(o2, o) and torch.equal(b2, b) and torch.equal(s2, s)
    assert aug.draw(B, DEV).step == 1
    # a resumed run repeats its draws
    again = TripletAugment("none")
    again.load_state_dict(dict(aug.state_dict(), step=0))
    p0 = again.draw(B, DEV)
    assert torch.equal(p0.ops, plan.ops) and torch.equal(p0.turb, plan.turb)
    with pytest.raises(ValueError, match="square"):
        aug.apply_one(plan, torch.zeros(B, 1, 8, 12, device=DEV))
    # mode "none" without turbidity: uint8 tiles come out as stage_tile_batch stages them
    none = TripletAugment("none", seed=1)
    o3, b3, s3 = none(opt, bathy, sss)
    assert torch.equal(o3, staging.stage_tile_batch(opt, True)) and b3 is bathy
    assert torch.equal(s3, staging.stage_tile_batch(sss, False))


# -------------------------------------------------------------------------------------- loop
def test_augmented_loader_through_the_training_loop(tmp_path, monkeypatch):
    import mauv.train as mt
    from mauv import AugmentedLoader, TripletAugment, dihedral
    from mauv.models import define_models, DEFAULT_PRIOR
    from tests.golden.common import make_batches, SEED_DATA
    from tests.helpers import ListLoader, NullWriter
    batches = make_batches(SEED_DATA, 2, B=2, S_opt=64, S_son=64)
    bare = ListLoader(batches, 2)
    # mode "none", no turbidity: the loop sees the bare loader's tensors
    none = AugmentedLoader(bare, TripletAugment("none", seed=1), DEV)
    assert len(none) == 2 and none.batch_size == 2
    for wb, bb in zip(none, bare):
        assert wb["main_image"].is_cuda and wb["label"] is bb["label"]
        for got, ref in zip(mt._batch_to(wb, DEV, None, None), mt._batch_to(bb, DEV, None, None)):
            assert torch.equal(got, ref)
    # "dihedral": one epoch runs, and the model receives the moved tensors
    torch.manual_seed(0)
    m = define_models(DEV, 7, DEFAULT_PRIOR)["multimodal_model"].to(DEV)
    seen, plans = [], []
    real_forward = type(m).mc_forward

    def recording_forward(self, inputs, bathy, sss, num_mc):
        seen.append((inputs.clone(), bathy.clone(), sss.clone()))
        return real_forward(self, inputs, bathy, sss, num_mc)

    monkeypatch.setattr(type(m), "mc_forward", recording_forward)
    aug = TripletAugment("dihedral", seed=2024)
    real_draw = aug.draw

    def recording_draw(B, device):
        plans.append(real_draw(B, device))
        return plans[-1]

    aug.draw = recording_draw
    opt = torch.optim.Adam(m.parameters(), lr=5e-5)
    csv_path = tmp_path / "run" / "train.csv"
    csv_path.parent.mkdir(parents=True)
    loss, acc = mt.train_multimodal_model(
        m, AugmentedLoader(bare, aug, DEV), torch.nn.CrossEntropyLoss(), opt, epoch=1, device=DEV,
        model_type="multimodal", total_num_epochs=2, num_mc=2, sum_writer=NullWriter(),
        csv_path=str(csv_path))
    assert np.isfinite(loss) and 0.0 <= acc <= 1.0
    assert len(seen) == 2 and len(plans) == 2 and [p.step for p in plans] == [0, 1]
    for got, batch, plan in zip(seen, batches, plans):
        for t, key in zip(got, ("main_image", "bathy_image", "sss_image")):
            assert torch.equal(t, dihedral(batch[key].to(DEV), plan.ops)), key
