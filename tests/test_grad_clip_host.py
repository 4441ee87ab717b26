"""Device-side gradient clipping, the part that needs no GPU: evp_grad_clip_multi is declared, exported and bound, validates its
arguments on the host before any launch, and FusedAdamW(max_grad_norm=...) leaves the checkpoint layout torch.optim.AdamW's."""
import ctypes
import math
import os
import re

import pytest
import torch

from conftest import ROOT

NAME = "evp_grad_clip_multi"


def test_grad_clip_entry_is_declared_exported_and_bound():
    from eventpretrain_amd import _lib
    txt = open(os.path.join(ROOT, "include", "evtpretrain.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int\s+" + NAME + r"\s*\(", txt, flags=re.S)
    assert m, NAME + " is not declared in include/evtpretrain.h"
    assert "utils/misc.py:289-290" in m.group(1)            # every entry cites the reference lines it replaces
    assert NAME in _lib.SIGNATURES and NAME in _lib.exported_symbols()
    assert len(_lib.SIGNATURES[NAME]) == 11 and _lib.SIGNATURES[NAME][7] is ctypes.c_double
    lib = _lib.load()
    assert hasattr(lib, NAME)
    assert lib.evp_abi_version() == _lib.ABI_VERSION == 5   # the change only adds
    # the entries beside it keep their signatures
    assert len(_lib.SIGNATURES["evp_adamw_multi"]) == 20 and len(_lib.SIGNATURES["evp_grad_norm_multi"]) == 9


def test_grad_clip_validates_arguments_before_any_launch():
    from eventpretrain_amd import _lib
    lib = _lib.load()
    fn = getattr(lib, NAME)
    buf = (ctypes.c_char * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p).value             # a non-null host address: validation never dereferences it
    good = [p, p, p, p, 1, 16384, p, 5.0, p, p, None]

    def bad(**kw):
        a = list(good)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return a

    cases = [bad(a0=None), bad(a1=None), bad(a2=None), bad(a3=None), bad(a6=None), bad(a8=None), bad(a9=None),
             bad(a4=0), bad(a4=-3),
             bad(a7=0.0), bad(a7=-1.0), bad(a7=math.inf), bad(a7=math.nan)]
    for a in cases:
        assert fn(*a) == -1, a                              # EVP_EINVAL
        msg = lib.evp_last_error()
        assert msg and NAME.encode() in msg, (a, msg)
    with pytest.raises(_lib.EvpError, match=NAME):
        _lib.call(NAME, *bad(a7=math.nan))


def test_fused_adamw_max_grad_norm_keeps_the_checkpoint_layout():
    from eventpretrain_amd.optim import FusedAdamW
    w, b = torch.nn.Parameter(torch.zeros(4, 3)), torch.nn.Parameter(torch.zeros(4))
    groups = lambda: [{"params": [w], "weight_decay": 0.05}, {"params": [b], "weight_decay": 0.0}]
    plain = FusedAdamW(groups(), lr=1e-3)
    assert plain.max_grad_norm is None and plain.last_grad_norm is None
    opt = FusedAdamW(groups(), lr=1e-3, max_grad_norm=5.0)
    assert opt.max_grad_norm == 5.0
    sd, sd0 = opt.state_dict(), plain.state_dict()
    assert sd.keys() == sd0.keys() == {"state", "param_groups"}
    assert [sorted(g) for g in sd["param_groups"]] == [sorted(g) for g in sd0["param_groups"]]
    assert all("max_grad_norm" not in g for g in sd["param_groups"])
    ref = torch.optim.AdamW(groups(), lr=1e-3)
    assert set(ref.state_dict()["param_groups"][0]) >= set(sd["param_groups"][0])
    other = FusedAdamW(groups(), lr=1e-3)
    other.load_state_dict(sd)
    assert other.max_grad_norm is None                       # a property of the run, not of the checkpoint
    opt.load_state_dict(sd0)
    assert opt.max_grad_norm == 5.0
    opt._parts = [None]
    with pytest.raises(Exception, match="max_grad_norm"):
        opt.launch_part(0)
