"""CPU: the C-ABI library loads and exports every symbol include/dq_hip.h declares; the ctypes table binds all of them
with matching arity (no compute calls -- there is no GPU here)."""
import ctypes
import os
import re

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "dq_hip.h")


def declared():
    src = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    out = {}
    for m in re.finditer(r"\b(dq_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.S):
        name, args = m.group(1), m.group(2).strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_header_symbols_exported_and_bound():
    from dquartic import _native as N

    decl = declared()
    assert len(decl) >= 16, decl
    lib = N.lib()
    for name, nargs in decl.items():
        assert hasattr(lib, name), f"{name} declared in dq_hip.h but not exported by libdq_hip.so"
        assert name in N.PROTOTYPES, f"{name} has no ctypes prototype"
        assert len(N.PROTOTYPES[name][1]) == nargs, f"{name}: header has {nargs} parameters, binding {len(N.PROTOTYPES[name][1])}"
    assert set(N.PROTOTYPES) == set(decl), set(N.PROTOTYPES) ^ set(decl)
    assert lib.dq_abi_version() == N.ABI_VERSION == 13  # DQ_ABI_VERSION in include/dq_hip.h


def record_fields():
    """the field names of the header's ``dq_sample_call`` typedef, in declaration order"""
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    body = re.search(r"typedef struct dq_sample_call \{(.*?)\} dq_sample_call;", src, flags=re.S).group(1)
    return [re.search(r"(\w+)$", decl.strip()).group(1) for decl in body.split(";") if decl.strip()]


def test_sample_call_layout_is_the_librarys():
    """``_native.SampleCall`` against ``dq_debug_sample_call_layout``: the total size, every field's offset and size, and the header's
    field names in order -- the check of the binding that needs no compiler"""
    from dquartic import _native as N

    size, fields = N.sample_call_layout()
    names = [k for k, _ in N.SampleCall._fields_]
    assert names == record_fields() and names[0] == "struct_bytes" and len(names) == 36
    assert size == ctypes.sizeof(N.SampleCall)
    assert fields == [(getattr(N.SampleCall, k).offset, getattr(N.SampleCall, k).size) for k in names]
    # fixed-width members only: 4-byte ints and floats, 8-byte pointers, int64 sizes and the one double
    assert all(n in (4, 8) for _, n in fields) and dict(zip(names, fields))["workspace_bytes"][1] == 8
    assert dict(N.SampleCall._fields_)["guidance_rescale"] is ctypes.c_double and dict(N.SampleCall._fields_)["struct_bytes"] is ctypes.c_int32
    lib = N.lib()
    small = (ctypes.c_int32 * 8)()
    assert lib.dq_debug_sample_call_layout(small, 8) == -1 and lib.dq_debug_sample_call_layout(None, 128) == -1


def test_sample_call_defaults():
    """``sample_call()``: struct_bytes set, every option at its off value (eta 0, null seed and ids, sampler 0, clip 0, guided 0, rescale
    and quantile 0, DQ_CONSIST_NONE with group_size 1), every other field zero; an unknown keyword raises"""
    from dquartic import _native as N

    q = N.sample_call()
    got = {k: getattr(q, k) for k, _ in N.SampleCall._fields_}
    want = {k: (None if t is ctypes.c_void_p else 0) for k, t in N.SampleCall._fields_}
    want.update(struct_bytes=ctypes.sizeof(N.SampleCall), group_size=1)
    assert got == want
    assert (q.eta, q.seed_dev, q.window_ids_dev, q.sampler, q.clip_x0, q.guided, q.guidance_rescale, q.threshold_quantile, q.consistency,
            q.group_size) == (0.0, None, None, 0, 0.0, 0, 0.0, 0.0, 0, 1)
    q = N.sample_call(B=3, eta=0.5, x_T=4096, seed_dev=None, guidance_rescale=0.1)
    assert (q.B, q.eta, q.x_T, q.seed_dev, q.guidance_rescale, q.group_size) == (3, 0.5, 4096, None, 0.1, 1)
    with pytest.raises(AttributeError, match="no field 'strength'"):
        N.sample_call(strength=1.0)


def test_a_record_of_another_size_is_refused_first():
    """both entries: a null record, then struct_bytes off by 4 either way, refused with both sizes in the message before any other field
    or argument is looked at (every other pointer is null here: the null-argument refusal would be next)"""
    from dquartic import _native as N

    lib, size = N.lib(), ctypes.sizeof(N.SampleCall)
    entries = {"dq_ddim_sample": lambda q: lib.dq_ddim_sample(None, None, None, q),
               "dq_tfm_sample": lambda q: lib.dq_tfm_sample(None, None, None, None, None, 0, q)}
    for who, entry in entries.items():
        assert entry(None) != 0 and lib.dq_last_error().startswith(f"{who}: null argument (call) [".encode())
        for off in (-4, 4):
            q = N.sample_call(struct_bytes=size + off)
            assert entry(ctypes.byref(q)) != 0
            err = lib.dq_last_error().decode()
            assert err.startswith(f"{who}: call->struct_bytes is {size + off}, sizeof(dq_sample_call) of this library is {size}"), err
        assert entry(ctypes.byref(N.sample_call())) != 0 and lib.dq_last_error().startswith(f"{who}: null argument [".encode())  # the next


def test_plan_layout_without_a_gpu():
    from dquartic import _native as N

    lib = N.lib()
    mults = (ctypes.c_int * 7)(1, 2, 2, 3, 3, 4, 4)
    plan = lib.dq_plan_create(4, 7, mults, 64, 1000)
    assert plan
    assert lib.dq_plan_num_params(plan) == 395 and lib.dq_plan_param_floats(plan) == 128847
    ws_inf = lib.dq_unet_workspace_bytes(plan, 32, 400, 0)
    ws_trn = lib.dq_unet_workspace_bytes(plan, 32, 400, 1)
    assert 0 < ws_inf and ws_trn == 2 * ws_inf
    lib.dq_plan_destroy(plan)
    # unsupported configurations fail loudly
    bad = (ctypes.c_int * 2)(1, 8)
    assert not lib.dq_plan_create(4, 2, bad, 64, 1000) and b"16" in lib.dq_last_error()
    assert not lib.dq_plan_create(4, 7, mults, 65, 1000) and b"divisible" in lib.dq_last_error()


def test_missing_library_raises(monkeypatch):
    from dquartic import _native as N

    monkeypatch.setattr(N, "_lib", None)
    monkeypatch.setattr(N, "LIB_PATH", "/nonexistent/libdq_hip.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        N.lib()
