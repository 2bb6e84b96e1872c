"""not-gpu: a compiled net that nobody holds any more gives its device buffers back (gr_net_destroy from the finaliser), but never after
its context was shut down (the net would point at freed memory).  The library is replaced by a stub that records the calls."""
import gc


class _StubLib:
    def __init__(self):
        self.destroyed = []

    def gr_net_destroy(self, h):
        self.destroyed.append(h)
        return 0


class _StubCtx:
    def __init__(self, lib, open_=True):
        self.lib, self.h = lib, (1234 if open_ else None)


def _net(ctx, h):
    import ganrev._lib as L
    n = object.__new__(L.Net)
    n.ctx, n.lib, n.h = ctx, ctx.lib, h
    return n


def test_dropped_net_is_destroyed_while_its_context_is_open():
    lib = _StubLib()
    n = _net(_StubCtx(lib), 77)
    del n
    gc.collect()
    assert lib.destroyed == [77]


def test_dropped_net_of_a_closed_context_is_left_alone_and_close_is_not_repeated():
    lib = _StubLib()
    n = _net(_StubCtx(lib, open_=False), 78)
    del n
    gc.collect()
    assert lib.destroyed == []
    m = _net(_StubCtx(lib), 79)
    m.close()
    del m
    gc.collect()
    assert lib.destroyed == [79]
