"""Skipping the optimizer step on non-finite gradients (reference utils/misc.py:290, GradScaler.step), the part that needs no GPU:
evp_grad_guard_multi and evp_adamw_guarded_multi are declared, exported and bound, validate their arguments on the host before any
launch, and FusedAdamW(skip_nonfinite=True) leaves the checkpoint layout torch.optim.AdamW's."""
import ctypes
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

from conftest import ROOT

GUARD, ADAMW = "evp_grad_guard_multi", "evp_adamw_guarded_multi"


def test_guard_entries_are_declared_exported_and_bound():
    from eventpretrain_amd import _lib
    txt = open(os.path.join(ROOT, "include", "evtpretrain.h")).read()
    for name in (GUARD, ADAMW):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+" + name + r"\s*\(", txt, flags=re.S)
        assert m, name + " is not declared in include/evtpretrain.h"
        assert "utils/misc.py:290" in m.group(1), name       # every entry cites the reference lines it replaces
        assert name in _lib.SIGNATURES and name in _lib.exported_symbols()
        assert hasattr(_lib.load(), name)
    assert "285-289" in re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+" + GUARD + r"\s*\(", txt, flags=re.S).group(1)     # the norm
    sig = _lib.SIGNATURES[GUARD]
    assert len(sig) == 14 and sig[7] is ctypes.c_double and sig[8] is ctypes.c_double and sig[9] is ctypes.c_double
    assert _lib.SIGNATURES[ADAMW] == _lib.SIGNATURES["evp_adamw_multi"][:-1] + [ctypes.c_void_p, ctypes.c_void_p]
    assert _lib.load().evp_abi_version() == _lib.ABI_VERSION == 5      # the change only adds
    assert len(_lib.SIGNATURES["evp_adamw_multi"]) == 20 and len(_lib.SIGNATURES["evp_grad_norm_multi"]) == 9
    assert len(_lib.SIGNATURES["evp_grad_clip_multi"]) == 11


def _cases(good, **groups):
    out = []
    for idx, values in groups.items():
        for v in values:
            a = list(good)
            a[int(idx[1:])] = v
            out.append(a)
    return out


def test_grad_guard_validates_arguments_before_any_launch():
    from eventpretrain_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value             # a non-null host address: validation never dereferences it
    good = [p, p, p, p, 1, 16384, p, 5.0, 0.9, 0.999, p, p, p, None]
    null = {"a%d" % i: [None] for i in (0, 1, 2, 3, 6, 10, 11, 12)}
    cases = _cases(good, a4=[0, -3], a5=[0, -4], a7=[-1.0, -1e-300, math.inf, -math.inf, math.nan],
                   a8=[0.0, 1.0, -0.1, 1.5, math.nan, math.inf], a9=[0.0, 1.0, -0.1, 1.5, math.nan, math.inf], **null)
    assert len(cases) == 8 + 4 + 5 + 12
    for a in cases:
        assert getattr(lib, GUARD)(*a) == -1, a             # EVP_EINVAL
        msg = lib.evp_last_error()
        assert msg and GUARD.encode() in msg, (a, msg)
    with pytest.raises(_lib.EvpError, match=GUARD):
        _lib.call(GUARD, *_cases(good, a8=[math.nan])[0])


def test_adamw_guarded_validates_arguments_before_any_launch():
    from eventpretrain_amd import _lib
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value
    good = [p, p, p, p, p, p, p, p, p, p, 1, 16384, 1.0, 0.9, 0.999, 1e-8, 1, 1.0, p, p, None]
    null = {"a%d" % i: [None] for i in (0, 1, 2, 3, 5, 6, 7, 8, 9, 18, 19)}      # (4, the bf16 shadow table, is optional)
    for a in _cases(good, a10=[0, -1], a11=[0, 6], a16=[0], **null):
        assert getattr(lib, ADAMW)(*a) == -1, a
        msg = lib.evp_last_error()
        assert msg and ADAMW.encode() in msg, (a, msg)
    # the entry beside it still names itself
    assert lib.evp_adamw_multi(*(good[:10] + [0] + good[11:19] + [None])) == -1 and b"evp_adamw_multi:" in lib.evp_last_error()


def _groups(w, b):
    return [{"params": [w], "weight_decay": 0.05}, {"params": [b], "weight_decay": 0.0}]


def test_fused_adamw_skip_nonfinite_keeps_the_checkpoint_layout():
    from eventpretrain_amd.optim import FusedAdamW
    w, b = torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(4))
    plain = FusedAdamW(_groups(w, b), lr=1e-3)
    assert plain.skip_nonfinite is False and plain.guard_state is None and plain.skipped_steps() == 0
    opt = FusedAdamW(_groups(w, b), lr=1e-3, skip_nonfinite=True)
    assert opt.skip_nonfinite is True and opt.max_grad_norm is None
    sd, sd0 = opt.state_dict(), plain.state_dict()
    assert sd.keys() == sd0.keys() == {"state", "param_groups"}
    assert [sorted(g) for g in sd["param_groups"]] == [sorted(g) for g in sd0["param_groups"]]
    assert all("skip_nonfinite" not in g for g in sd["param_groups"])
    ref = torch.optim.AdamW(_groups(w, b), lr=1e-3)
    assert set(ref.state_dict()["param_groups"][0]) >= set(sd["param_groups"][0])
    other = FusedAdamW(_groups(w, b), lr=1e-3)
    other.load_state_dict(sd)
    assert other.skip_nonfinite is False                      # a property of the run, not of the checkpoint
    opt.load_state_dict(sd0)
    assert opt.skip_nonfinite is True
    opt._parts = [None]
    with pytest.raises(Exception, match="skip_nonfinite"):
        opt.launch_part(0)


def test_executor_and_loops_take_the_option_and_refuse_what_cannot_guard():
    from eventpretrain_amd import engine
    from eventpretrain_amd.optim import FusedAdamW
    from eventpretrain_amd.trainer import epoch as ep
    w = torch.nn.Parameter(torch.zeros(3))
    sgd = torch.optim.SGD([w], lr=0.1)
    with pytest.raises(ValueError, match="skip_nonfinite"):
        engine.GraphedStep(None, sgd, None, [torch.zeros(1)], use_graph=False, skip_nonfinite=True)
    args = SimpleNamespace(skip_nonfinite=True)
    with pytest.raises(ValueError, match="FusedAdamW"):
        ep.run_epoch(args, None, [], sgd, 0, None, None, ("loss",), None)
    opt = FusedAdamW([w], lr=1e-3)
    with pytest.raises(ValueError, match="step_executor"):
        ep.run_epoch(args, None, [], opt, 0, None, None, ("loss",), None, step_executor=SimpleNamespace(skip_nonfinite=False))
    assert opt.skip_nonfinite is False
