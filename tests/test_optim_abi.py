"""not-gpu: the ABI of the fused sgd | adagrad | adadelta | adamax | rmsprop step (gr_optim_step, include/ganrev.h): the ctypes and LuaJIT twins of
gr_optim_config have the header's layout, the binding's defaults are the defaults of the float32 mirrors in ganrev/optim.py (the specification of
the device kernels), and the refusals return a status instead of launching."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = {"int32_t": 4, "double": 8}
CTYPES = {"int32_t": C.c_int32, "double": C.c_double}


def _struct_fields(txt, name):
    """[(type, field)] of `typedef struct { ... } name;` in a piece of C, comments dropped"""
    txt = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + name + r"\s*;", txt).group(1)
    out = []
    for decl in body.split(";"):
        if decl.strip():
            typ, names = decl.strip().split(" ", 1)
            out += [(typ, n.strip()) for n in names.split(",")]
    return out


def _header():
    return open(os.path.join(ROOT, "include", "ganrev.h")).read()


def _lib():
    import __graft_entry__ as g
    g.build()
    import ganrev._lib as L
    return L, L.load_library()


def test_optim_config_layout_is_the_headers_in_ctypes_and_in_the_lua_cdef():
    import ganrev._lib as L
    fields = _struct_fields(_header(), "gr_optim_config")
    assert [f for _, f in fields] == [f for f, _ in L.OptimConfig._fields_]
    offset = 0
    for (typ, name), (_, ctype) in zip(fields, L.OptimConfig._fields_):
        assert ctype is CTYPES[typ], name
        offset = -(-offset // SIZES[typ]) * SIZES[typ]              # C: every member aligned to its own size
        assert getattr(L.OptimConfig, name).offset == offset, (name, getattr(L.OptimConfig, name).offset, offset)
        offset += SIZES[typ]
    assert C.sizeof(L.OptimConfig) == -(-offset // 8) * 8 == 2 * 4 + 14 * 8
    lua = open(os.path.join(ROOT, "gan-reverser_amd", "lua", "hipnn.lua")).read()
    cdef = re.search(r"ffi\.cdef\[\[(.*?)\]\]", lua, flags=re.S).group(1)
    assert _struct_fields(cdef, "gr_optim_config") == fields
    # the method numbers: header, binding and the Lua wrapper's table
    hdr = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    numbers = {k.lower(): int(v) for k, v in re.findall(r"GR_OPT_([A-Z]+) = (\d+)", hdr)}
    assert numbers == L.OPT_METHODS == {"sgd": 1, "adagrad": 2, "adadelta": 3, "adamax": 4, "rmsprop": 5}
    table = re.search(r"local OPT_METHODS = \{([^}]*)\}", lua).group(1)
    assert {k: int(v) for k, v in re.findall(r"(\w+)=(\d+)", table)} == numbers


@pytest.mark.parametrize("method", ["sgd", "adagrad", "adadelta", "adamax", "rmsprop"])
def test_optim_config_defaults_are_the_mirrors_defaults(method):
    """An empty table through OptimConfig spells out the values the mirror takes for absent keys: the mirror run on the empty table and on
    the spelled-out one takes the same three steps, bit for bit (a float64 default that differed would show in the float32 scalars)."""
    import ganrev._lib as L
    from ganrev import optim
    cfg = L.OptimConfig(method)
    assert cfg.method == L.OPT_METHODS[method] and (cfg.l1, cfg.l2, cfg.clamp) == (0.0, 0.0, 0.0)
    spelled = {name: getattr(cfg, name) for name, _ in L.OptimConfig._fields_ if name not in ("method", "nesterov", "l1", "l2", "clamp")}
    spelled["nesterov"] = bool(cfg.nesterov)
    rng = np.random.default_rng(11)
    xs = [rng.standard_normal(33).astype(np.float32) for _ in range(2)]
    xs[1][...] = xs[0]
    states = [{}, spelled]
    for step in range(3):
        g = rng.standard_normal(33).astype(np.float32)
        for x, st in zip(xs, states):
            optim.METHODS[method](lambda _: (0.0, g.copy()), x, st)
        assert np.array_equal(xs[0], xs[1]), (method, step)
    assert L.OptimConfig("sgd", {"momentum": 0.5}).dampening == 0.5 and L.OptimConfig("sgd", {"momentum": 0.5, "dampening": 0.0}).dampening == 0.0
    assert L.OptimConfig("sgd", {"learningRate": 0.02, "momentum": 0.0}).slots() == (False, False)        # train.lua:189-190: no state at all
    assert L.OptimConfig("sgd", {"momentum": 0.5}).slots() == (True, False) and L.OptimConfig("adamax").slots() == (True, True)
    assert L.OptimConfig("adadelta").slots() == (True, True) and L.OptimConfig("rmsprop").slots() == L.OptimConfig("adagrad").slots() == (True, False)


def test_optim_step_refuses_with_a_status():
    """gr_optim_step / gr_optim_reset / gr_optim_get_state / gr_optim_set_state exist and answer GR_ERR_INVALID, not an abort: an unknown method,
    a nesterov request without momentum or with dampening, a null net or config.  (No net exists without a GPU, so every call here also has the
    null net: tests/test_gpu_optim.py repeats the first two on a live net, where the message names the reason and nothing is launched.)"""
    L, lib = _lib()
    INVALID = -1
    assert L.STATUS[INVALID] == "GR_ERR_INVALID"
    for cfg in (L.OptimConfig(99), L.OptimConfig(0), L.OptimConfig("sgd", {"nesterov": True}),
                L.OptimConfig("sgd", {"nesterov": True, "momentum": 0.5}), L.OptimConfig("sgd")):
        assert lib.gr_optim_step(None, C.byref(cfg), 1) == INVALID
    assert lib.gr_optim_step(None, None, 1) == INVALID
    assert lib.gr_optim_reset(None) == INVALID
    assert lib.gr_optim_get_state(None, None, None) == INVALID and lib.gr_optim_set_state(None, None, None) == INVALID
    with pytest.raises(L.GanrevError, match="Unknown optimizer method 'lbfgs'"):
        L.OptimConfig("lbfgs")


def test_device_game_names_an_unknown_method_as_the_reference_does():
    """adversarial.lua:170,197: error("Unknown optimizer method '%s' chosen for D.") - raised before anything touches the GPU"""
    import ganrev._lib as L
    from ganrev import adversarial, models
    G, D = models.create_G((1, 16, 16), 8), models.create_D2((1, 16, 16))
    for which in ("D", "G"):
        env = adversarial.make_env(G, D, (1, 16, 16), batchSize=8, noiseDim=8, **{which + "_optmethod": "lbfgs"})
        with pytest.raises(L.GanrevError, match=f"Unknown optimizer method 'lbfgs' chosen for {which}."):
            adversarial.DeviceGame(env)
