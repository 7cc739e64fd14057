"""Call-level timing of the on-device triplet augmentation on the bench's
configs[1] batch: B = 64 decoded uint8 tiles of 256 x 256 with C = 3 (optical), 3 (bathymetry)
and 1 (side-scan).  All arms run interleaved in one process, `--repeats` times in rotated
order, each after `--warmup` calls, timed with device events over `--steps` calls:

  a        stage_tile_batch of the three tiles: the un-augmented input path
  b        TripletAugment("dihedral", turbidity=(0.3, 1.5)) on the same tiles (draw + apply)
  b_flips  the same in "flips" mode (no transposing code): tells the gather's share of b
  c        what a user writes without it: a (the optical tile with the scalar degradation fused
           in), then a per-item torch.flip / transpose loop over the B items of each modality
  d        clone() of the three fp32 outputs: one extra read-and-write pass
  e_aug    fp32 NCHW inputs (what the host datasets hand over): the three stage_f32_aug passes
  e_clone  clone() of the same three fp32 tensors

Two conditions, both against code that is not under test:  b < c,  and  b <= a + d  (a design of
"stage, then a separate move pass" would reach a + d).  Each verdict compares the means and
prints the difference beside the spread (max - min) of the repeats of the arms involved; a
difference inside that spread is marked as not resolved.  Raw times go to `--out` as JSON.

    python tools/augment_time.py [--repeats 3] [--warmup 20] [--steps 200] [--out DIR]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-auv_amd")]
import torch  # noqa: E402

from mauv import TripletAugment, staging  # noqa: E402

ARMS = ("a", "b", "b_flips", "c", "d", "e_aug", "e_clone")


def user_move(x, codes):
    """The per-item loop a user writes today (host-side codes, up to 3 small launches per item
    and a stack)."""
    out = []
    for xb, k in zip(x, codes):
        if k & 2:
            xb = xb.flip(-2)
        if k & 1:
            xb = xb.flip(-1)
        if k & 4:
            xb = xb.transpose(-2, -1)
        out.append(xb)
    return torch.stack(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "augment"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("augment_time.py measures on a ROCm GPU; there is none (not measured)")
    dev = torch.device("cuda", 0)
    B, S = a.batch, a.size
    g = torch.Generator().manual_seed(1234)
    opt, bathy, sss = (torch.randint(0, 256, (B, S, S, C), generator=g, dtype=torch.uint8).to(dev)
                       for C in (3, 3, 1))
    stage = staging.stage_tile_batch
    f_opt, f_bathy, f_sss = stage(opt, True), stage(bathy, False), stage(sss, False)
    aug = TripletAugment("dihedral", turbidity=(0.3, 1.5), seed=2024)
    flips = TripletAugment("flips", turbidity=(0.3, 1.5), seed=2024)
    host_codes = torch.randint(0, 8, (B,), generator=g).tolist()

    def arm_c():
        o = staging.resize_to_tensor(opt, staging.TILE_SIZE, staging.OPTICAL_MEAN,
                                     staging.OPTICAL_STD, degrade=(0.9, 1.0))
        return (user_move(o, host_codes), user_move(stage(bathy, False), host_codes),
                user_move(stage(sss, False), host_codes))

    fns = {
        "a": lambda: (stage(opt, True), stage(bathy, False), stage(sss, False)),
        "b": lambda: aug(opt, bathy, sss),
        "b_flips": lambda: flips(opt, bathy, sss),
        "c": arm_c,
        "d": lambda: (f_opt.clone(), f_bathy.clone(), f_sss.clone()),
        "e_aug": lambda: aug(f_opt, f_bathy, f_sss),
        "e_clone": lambda: (f_opt.clone(), f_bathy.clone(), f_sss.clone()),
    }
    # the augmented path computes what the plain path computes, moved (checked once, untimed)
    o, b_, s_ = aug(opt, bathy, sss)
    from mauv import dihedral
    assert torch.equal(b_, dihedral(f_bathy, aug.last_plan.ops))
    assert torch.equal(s_, dihedral(f_sss, aug.last_plan.ops))
    del o, b_, s_

    res = {k: [] for k in ARMS}
    for r in range(a.repeats):
        order = ARMS[r % len(ARMS):] + ARMS[:r % len(ARMS)]
        for name in order:
            fn = fns[name]
            for _ in range(a.warmup):
                fn()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) / a.steps * 1e3
            res[name].append(us)
            print(f"repeat {r} {name:8s}: {us:9.1f} us/call", flush=True)
    mean = {k: sum(v) / len(v) for k, v in res.items()}
    spread = {k: max(v) - min(v) for k, v in res.items()}
    out_bytes = B * S * S * 7 * 4
    print(f"\nB = {B}, {S} x {S}, C = 3 / 3 / 1; fp32 output {out_bytes / 1e6:.1f} MB per call; "
          f"{a.repeats} repeats x {a.steps} calls, device events")
    print("| arm | us/call (repeats) | mean | spread |\n|---|---|---|---|")
    for k in ARMS:
        print(f"| {k} | " + " ".join(f"{v:.1f}" for v in res[k]) +
              f" | {mean[k]:.1f} | {spread[k]:.1f} |")
    # one convention for both: the verdict compares the means; the spread of the arms involved
    # is printed beside the difference, and a difference inside it is called out as such
    def verdict(name, lhs, rhs, margin, strict):
        ok = lhs < rhs if strict else lhs <= rhs
        close = " (inside the spread: not resolved by this run)" if abs(rhs - lhs) <= margin else ""
        print(f"{name}: {lhs:.1f} vs {rhs:.1f} us, difference {rhs - lhs:+.1f}, spread "
              f"{margin:.1f}: {'PASS' if ok else 'FAIL'}{close}")
        return ok

    ok1 = verdict("b < c", mean["b"], mean["c"], max(spread["b"], spread["c"]), True)
    ok2 = verdict("b <= a + d", mean["b"], mean["a"] + mean["d"],
                  max(spread["b"], spread["a"] + spread["d"]), False)
    print(f"e: stage_f32_aug {mean['e_aug']:.1f} vs clone {mean['e_clone']:.1f} us")
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "augment_time.json"), "w") as fh:
        json.dump({"device": torch.cuda.get_device_name(0), "batch": B, "size": S,
                   "repeats": a.repeats, "warmup": a.warmup, "steps": a.steps, "unit": "us/call",
                   "times": res, "mean": mean, "spread": spread,
                   "b_lt_c": ok1, "b_le_a_plus_d": ok2}, fh, indent=1)
    return 0 if ok1 and ok2 else 1


if __name__ == "__main__":
    sys.exit(main())
