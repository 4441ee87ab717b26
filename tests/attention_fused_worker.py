"""Child process of tests/test_gpu_attention_truth.py: the attention kernels on one group of attention_truth's cases, through the
gates and guards. The cases run here and not in the suite's own process for two reasons: the wave counts that EVP_ATTN_FWD_WAVES /
EVP_ATTN_BWD_WAVES select are read once per process, at the library's first launch; and running the cases inside the suite's
process was measured to shorten the eager epoch loop that a later test of the suite times against the captured loop
(tests/test_gpu_round3.py: 11.8 ms per step instead of 14.3), which running them in children does not.

    python tests/attention_fused_worker.py edges | heads | peaked | waves | single_token | win_edge | win_walk | win_single_token | unfused

Exit status 0 when every gate, guard and identity holds, 1 otherwise."""
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

import attention_truth as at  # noqa: E402

GROUPS = {"edges": (at.FUSED_VIT, (False, True)), "heads": (at.HEAD_MAP_CASES, (True,)), "peaked": (at.PEAKED, (True,)),
          "waves": (at.WAVES, (True,))}
U23 = 2.0 ** -23


def single_token(dh):
    """N = 1: P = 1, so out is the v slice and dv is dout, bit for bit; lse = q.k * scale within f32 rounding; dq = dk = 0 in truth.
    The kernel forms dS = P * (dP - delta) * scale with dP = dout . v from the MFMA and delta = dout . out (out = v here) from its
    staging code: two f32 sums of the SAME d_h exact products (bf16 x bf16 is exact in f32) in different orders. Each sum of n terms
    is off by at most (n - 1) u * sum|terms| for any order, u = 2^-23 covering round-to-nearest and a truncating accumulator alike, so
    |dP - delta| <= 2 (d_h - 1) u sum_i |dout_i v_i|; P <= 1 + 2^-8 after its rounding to bf16, dS and the result are rounded to bf16
    once each (1 + 2^-8 each), hence |dq_j| <= 1.02 * scale * 2 (d_h - 1) u * sum_i |dout_i v_i| * |k_j|, and dk likewise with q."""
    name = at.vit_name(2, 2, 1, dh)
    c = at.make_case(name)
    _, raw = at.run_fused_vit(name, True)
    B, h = c["Bt"], c["heads"]
    q, k, v = c["qkv"].view(B, 3, h, dh).unbind(1)
    do = c["dout"].view(B, h, dh)
    assert torch.equal(raw["out"].view(B, h, dh), v), "out is not the v slice"
    d = raw["dqkv"].view(B, 3, h, dh)
    assert torch.equal(d[:, 2], do), "dv is not dout"
    assert torch.equal(raw["probs"][..., 0].view(B, h).float(), torch.ones(B, h)), "P is not 1"
    want = (q.double() * k.double()).sum(-1) * c["scale"]
    tol = (dh + 2) * U23 * (q.double() * k.double()).abs().sum(-1) * c["scale"]
    assert ((raw["lse"].view(B, h).double() - want).abs() <= tol).all(), "lse off q.k * scale"
    bound = 1.02 * c["scale"] * 2 * (dh - 1) * U23 * (do.double() * v.double()).abs().sum(-1, keepdim=True)
    assert (d[:, 0].double().abs() <= bound * k.double().abs()).all(), "dq over the summation-order bound"
    assert (d[:, 1].double().abs() <= bound * q.double().abs()).all(), "dk over the summation-order bound"
    print(f"single token d_h = {dh}: identities hold, max |dq| {float(d[:, 0].abs().max()):.2e}, max |dk| {float(d[:, 1].abs().max()):.2e}")


def main(group):
    print("group:", group, {k: os.environ.get(k) for k in ("EVP_ATTN_FWD_WAVES", "EVP_ATTN_BWD_WAVES")})
    bad, worst = [], (0.0, "")
    if group == "single_token":
        jobs = [(f"single_token d_h={dh}", lambda dh=dh: single_token(dh) or ([], (0.0, ""))) for dh in (32, 64)]
    elif group in ("win_edge", "win_walk", "win_single_token", "unfused"):
        import test_gpu_attention_truth as tg
        jobs = {"win_edge": [(n, lambda n=n: tg.window_edge(n)) for n in at.WIN_EDGE],
                "win_walk": [(at.win_name(*w[:4]), lambda w=w: tg.window_walk(*w)) for w in at.WIN_WALK],
                "win_single_token": [("window single token", lambda: tg.window_single_token() or ([], (0.0, "")))],
                "unfused": [(n, lambda n=n: tg.unfused(n)) for n in at.UNFUSED]}[group]
    else:
        names, modes = GROUPS[group]
        jobs = [(f"{n} probs={int(p)}", lambda n=n, p=p: at.gate_report(n, at.run_fused_vit(n, p)[0], f"{n} probs={int(p)}")) for n in names for p in modes]
    for what, job in jobs:
        try:
            fails, w = job()
            bad += fails
            worst = max(worst, (w[0], f"{what}: {w[1]}"))
        except AssertionError:
            bad.append(f"{what}: {traceback.format_exc()}")
    print(f"\n[{group}] worst of the group {worst[0]:.2f} at {worst[1]}")
    print("\n".join(bad) if bad else "all gates hold")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
