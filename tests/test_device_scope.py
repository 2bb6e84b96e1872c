"""nn_utils.DeviceScope and nn_utils.deviceTable on a context that only records what is asked of it: who frees what, when, and how often."""
import numpy as np
import pytest


class FakeContext:
    def __init__(self):
        self.calls, self.live, self.next = [], set(), 0x1000

    def malloc(self, nbytes):
        self.next += 0x1000
        self.live.add(self.next)
        self.calls.append(("malloc", self.next))
        return self.next

    def upload(self, arr, dptr=None):
        arr = np.ascontiguousarray(arr)
        self.uploaded = arr
        return self.malloc(arr.nbytes) if dptr is None else dptr

    def free(self, p):
        assert p in self.live, f"{p:#x} freed twice, or never handed out"
        self.live.remove(p)
        self.calls.append(("free", p))

    def synchronize(self):
        self.calls.append(("synchronize", None))

    def freed(self):
        return [p for what, p in self.calls if what == "free"]


class Closable:
    def __init__(self, log, name):
        self.log, self.name = log, name

    def close(self):
        self.log.append(self.name)


def test_scope_releases_in_reverse_order_each_once():
    from ganrev.nn_utils import DeviceScope, DeviceTensor
    ctx, log = FakeContext(), []
    with DeviceScope(ctx) as scope:
        a = scope.tensor((4, 3))
        b = scope.malloc(64)
        c = scope.upload(np.zeros(5, np.float32))
        d = scope.adopt(DeviceTensor(ctx, (2,)))
        e = scope.adopt(Closable(log, "axes"))
        pa, pd = a.ptr, d.ptr
        assert isinstance(a, DeviceTensor) and a.shape == (4, 3) and isinstance(b, int) and isinstance(c, int) and len(ctx.live) == 4
    assert log == ["axes"] and ctx.freed() == [pd, c, b, pa] and not ctx.live
    assert a.ptr is None and d.ptr is None and e.name == "axes"


def test_scope_early_release_is_the_only_release():
    from ganrev.nn_utils import DeviceScope
    ctx = FakeContext()
    with DeviceScope(ctx) as scope:
        a, b, raw = scope.tensor((8,)), scope.tensor((8,)), scope.malloc(16)
        pa, pb = a.ptr, b.ptr
        scope.release(a)
        scope.release(raw)
        assert ctx.freed() == [pa, raw] and a.ptr is None and ctx.live == {pb}
        scope.release(a)                                    # a second time: nothing
        scope.release(None)                                 # what was never handed out: nothing
        assert ctx.freed() == [pa, raw]
    assert ctx.freed() == [pa, raw, pb] and not ctx.live    # FakeContext.free asserts that nothing goes twice


def test_scope_releases_on_exception_and_lets_it_through():
    from ganrev.nn_utils import DeviceScope
    ctx = FakeContext()
    with pytest.raises(KeyError, match="step failed"):
        with DeviceScope(ctx) as scope:
            scope.tensor((8,)); scope.upload(np.ones(3, np.float32))
            raise KeyError("step failed")
    assert len(ctx.freed()) == 2 and not ctx.live


def test_scope_close_empties_it_before_the_block_ends():
    from ganrev.nn_utils import DeviceScope
    ctx = FakeContext()
    with DeviceScope(ctx) as scope:
        scope.tensor((8,)); scope.tensor((8,))
        scope.close()
        assert not ctx.live and len(ctx.freed()) == 2
        late = scope.tensor((2,))
    assert late.ptr is None and len(ctx.freed()) == 3 and not ctx.live


def test_device_tensor_is_a_context_manager():
    from ganrev.nn_utils import DeviceTensor
    ctx = FakeContext()
    with pytest.raises(ValueError):
        with DeviceTensor(ctx, (3, 3)) as t:
            p = t.ptr
            view = t.rows(1, 2)
            with view:                                      # a view owns nothing
                pass
            assert ctx.live == {p}
            raise ValueError
    assert ctx.freed() == [p] and t.ptr is None


def test_device_table_of_a_host_array_synchronises_then_frees():
    from ganrev.nn_utils import deviceTable
    ctx = FakeContext()
    table = np.arange(24, dtype=np.float64).reshape(6, 4)
    with deviceTable(ctx, table) as (ptr, N, d):
        assert (N, d) == (6, 4) and ctx.live == {ptr} and ctx.uploaded.dtype == np.float32 and ctx.uploaded.shape == (6, 4)
    assert ctx.calls == [("malloc", ptr), ("synchronize", None), ("free", ptr)]
    ctx = FakeContext()
    with deviceTable(ctx, table, rows=2) as (ptr, N, d):    # the map's prefix
        assert (N, d) == (2, 4) and np.array_equal(ctx.uploaded, table[:2].astype(np.float32))
    with pytest.raises(RuntimeError):
        with deviceTable(ctx, table) as (ptr, N, d):
            raise RuntimeError
    assert ctx.calls[-2:] == [("synchronize", None), ("free", ptr)] and not ctx.live


def test_device_table_of_a_device_tensor_does_neither():
    from ganrev.nn_utils import DeviceTensor, deviceTable
    ctx = FakeContext()
    t = DeviceTensor(ctx, (6, 2, 2))
    before = list(ctx.calls)
    with deviceTable(ctx, t) as (ptr, N, d):
        assert (ptr, N, d) == (t.ptr, 6, 4)
    with deviceTable(ctx, t, rows=3) as (ptr, N, d):
        assert (ptr, N, d) == (t.ptr, 3, 4)
    assert ctx.calls == before and ctx.live == {t.ptr}
