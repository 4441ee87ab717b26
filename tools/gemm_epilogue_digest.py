#!/usr/bin/env python3
"""One SHA-256 per evp_gemm epilogue case, of C and of the stored pre-activation where one is written: run it from two checkouts on
the same GPU and compare the lists line by line. The library is built with -ffp-contract=off and nothing here uses split-K (no
atomics), so a change that keeps the order of the epilogue's floating-point operations keeps every digest.

Covers operands in bf16 / f32, C in bf16 / f32, tiles 1, 2, 4 (128-class) and 20-22 (G4) where the kernels admit them, every epilogue
in CASES, a shape with whole and ragged tiles in M and N, and one whose N is no multiple of 4 (the scalar edge; C has padding columns,
which are hashed too and must come back untouched). tests/test_gpu_gemm.py takes its epilogue cases from here."""
import collections
import hashlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from eventpretrain_amd import ops  # noqa: E402
from eventpretrain_amd._lib import ACT_DGELU, ACT_DRELU, ACT_GELU, ACT_NONE, ACT_RELU  # noqa: E402

# aux: the pre-activation, stored by an activation forward and read by an activation backward (transB layout)
Case = collections.namedtuple("Case", "name act bias residual accumulate aux")
CASES = [
    Case("linear", ACT_NONE, False, False, False, False),
    Case("linear+bias", ACT_NONE, True, False, False, False),
    Case("linear+res", ACT_NONE, False, True, False, False),
    Case("linear+bias+res", ACT_NONE, True, True, False, False),
    Case("linear+acc", ACT_NONE, False, False, True, False),
    Case("linear+bias+res+acc", ACT_NONE, True, True, True, False),
    Case("gelu", ACT_GELU, True, False, False, False),
    Case("gelu+aux", ACT_GELU, True, False, False, True),
    Case("gelu+res", ACT_GELU, True, True, False, False),
    Case("gelu+aux+res", ACT_GELU, True, True, False, True),
    Case("relu", ACT_RELU, True, False, False, False),
    Case("dgelu", ACT_DGELU, False, False, False, True),
    Case("drelu", ACT_DRELU, False, False, False, True),
]
ALPHA = 0.5
FILL = 7.0          # what C and a stored pre-activation hold before the launch


def admits(case, dtype, c_dtype, tile):
    """What evp_gemm builds: bf16 C needs bf16 operands, accumulate an f32 C; tile 4 and the G4 tiles are bf16 only, and the G4 tiles
    write bf16 C without residual / accumulate."""
    if dtype == torch.float32 and (c_dtype != torch.float32 or tile not in (1, 2)):
        return False
    if case.accumulate and c_dtype != torch.float32:
        return False
    if tile >= 20 and (c_dtype != torch.bfloat16 or case.residual or case.accumulate):
        return False
    return True


def problem(M, N, K, ldc, dtype, seed):
    """Operands of one shape on the device, drawn on the CPU from a fixed seed. C, aux and the residual share the row stride ldc."""
    gen = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=gen).to(dtype)
    b = torch.randn(N, K, generator=gen).to(dtype)
    bt = torch.zeros(K, ldc, dtype=dtype)
    bt[:, :N] = b.t()
    p = dict(M=M, N=N, K=K, ldc=ldc, dtype=dtype, a=a, b=b, bt=bt, bias=torch.randn(N, generator=gen),
             res=torch.randn(M, ldc, generator=gen), c0=torch.randn(M, ldc, generator=gen), h=torch.randn(M, ldc, generator=gen))
    return {k: v.cuda() if torch.is_tensor(v) else v for k, v in p.items()}


def run(case, p, c_dtype, tile):
    """-> (C, aux or None) as full [M, ldc] device tensors; aux is None unless this launch wrote it."""
    M, N, K, ldc = p["M"], p["N"], p["K"], p["ldc"]
    backward = case.act in (ACT_DGELU, ACT_DRELU)
    c = (p["c0"] if case.accumulate else torch.full((M, ldc), FILL, device="cuda")).to(c_dtype, copy=True)
    aux = None
    if case.aux:
        aux = p["h"].to(c_dtype) if backward else torch.full((M, ldc), FILL, dtype=c_dtype, device="cuda")
    ops.gemm(p["a"], p["bt"] if backward else p["b"], c, M=M, N=N, K=K, trans_b=backward, ldb=ldc if backward else K, ldc=ldc,
             alpha=ALPHA, bias=p["bias"] if case.bias else None, act=case.act, aux=aux, residual=p["res"] if case.residual else None,
             accumulate=case.accumulate, tile=tile)
    return c, (None if backward else aux)


def digest(t):
    return hashlib.sha256(t.contiguous().view(torch.uint8).cpu().numpy().tobytes()).hexdigest()


def main():
    small = [(200, 136, 96, 136), (200, 134, 96, 136)]
    for dtype in (torch.bfloat16, torch.float32):
        for tiles, shapes in (((1, 2, 4), small), ((20, 21, 22), [(520, 520, 128, 520)])):
            for (M, N, K, ldc) in shapes:
                p = problem(M, N, K, ldc, dtype, seed=1000 + N)
                for c_dtype in (torch.bfloat16, torch.float32):
                    for tile in tiles:
                        for case in CASES:
                            if not admits(case, dtype, c_dtype, tile):
                                continue
                            c, aux = run(case, p, c_dtype, tile)
                            pad = p["c0"] if case.accumulate else torch.full_like(p["c0"], FILL)
                            assert torch.equal(c[:, N:].float(), pad[:, N:]), "wrote outside N"
                            assert aux is None or bool((aux[:, N:].float() == FILL).all()), "aux written outside N"
                            tag = f"{M}x{N}x{K} ldc={ldc} {str(dtype)[6:]}->{str(c_dtype)[6:]} tile={tile} {case.name}"
                            print(f"{tag:64s} C {digest(c)}" + (f" aux {digest(aux)}" if aux is not None else ""), flush=True)


if __name__ == "__main__":
    main()
