"""CPU: the per-shape buffer scopes of frcnn_hip.runtime.Session (round 6; VERDICT r5 "missing 1").  The reference's graph takes any
[1, H, W, 3] image and test_net walks an imdb of hundreds of sizes (lib/nets/network.py:386-390, lib/model/test.py:138-185); here every
shape owns static buffers, so the session keeps them per shape and least-recently-used: what is tested is the bookkeeping -- which store
a buffer request lands in, what an eviction drops (buffers, the captured graph, recorded steps that address the buffers, a running
stream search), that weight-shaped buffers stay with the session, and that scratch follows the scope.  The device behaviour (memory
bounded over 64 shapes, bit-identical detections) is tests/test_streaming_shapes_gpu.py."""
import pytest
import torch

from frcnn_hip import ops, replay
from frcnn_hip.runtime import Session


def _host_session():
    s = Session.__new__(Session)                     # (Session() needs a GPU; the bookkeeping does not)
    s._init_host(torch.device("cpu"), 3)
    return s


@pytest.fixture
def sess(monkeypatch):
    s = _host_session()
    s.synced = []
    monkeypatch.setattr(torch.cuda, "synchronize", lambda device=None: s.synced.append(device))
    assert ops.scope_depth() == 0
    yield s
    del ops._scope_stack[1:]


def test_requests_land_in_the_active_scope_and_the_session_otherwise(sess):
    g = sess.buf("w", (4,))
    with sess.shape_scope("A", group="t", cap=2):
        a = sess.buf("act", (8,))
        assert sess.buf("act", (8,)) is a and sess.buf("w", (4,)) is not g          # same name inside a scope: the scope's own buffer
        with ops.unscoped():
            assert sess.buf("w", (4,)) is g                                          # weight-shaped: the session's
        ws = ops.workspace(100, sess.device, "x")
        assert ops.workspace(50, sess.device, "x") is ws
        big = ops.workspace(200, sess.device, "x")                                   # grows: the old one is retired INTO the scope
        assert big is not ws and sess.scopes["A"][("ws_retired",)] == [ws]
    assert ops.scope_depth() == 0
    assert set(sess.buffers) == {("w", (4,), torch.float32)}
    assert ("act", (8,), torch.float32) in sess.scopes["A"] and sess.scope_bytes("A") >= 8 * 4 + 4 * 4 + 200
    with sess.shape_scope("A", group="t", cap=2):
        assert sess.buf("act", (8,)) is a                                            # re-entered: the same buffers (a captured graph addresses them)
    outside = ops.workspace(10, sess.device, "x")
    assert outside is not big                                                        # outside a scope: the module-wide scratch, as before


def test_lru_eviction_drops_buffers_graphs_and_recordings_together(sess):
    class Picker(object):
        done = False
    for i, k in enumerate(["A", "B", "C"]):
        with sess.shape_scope(k, group="t", cap=3):
            sess.buf("act", (16 * (i + 1),))
        sess.graphs[k] = replay.CapturedGraph(k, "graph", None, 0, 0, None)          # forward_device's entry: its scope is its own key
        sess.graphs[("propose", k)] = replay.CapturedGraph(k, "graph", None, 0, 0, None)    # propose_device's names the same scope
    for n, k in ((1, "A"), (2, "B")):
        sess.graphs[("train_replay", n)] = replay.RecordedStep(k)
        sess.graphs[("train_replay", n)].rec = "r%d" % n
    sess.graphs[("train_replay", 1)].picker = Picker()
    with sess.shape_scope("other", group="u", cap=1):                                # another group: counts separately
        sess.buf("act", (4,))
    sess.picking = True
    with sess.shape_scope("A", group="t", cap=3):                                    # touch A: B is now the least recently used of group t
        pass
    assert sess.synced == []
    with sess.shape_scope("D", group="t", cap=3):
        sess.buf("act", (4,))
    assert len(sess.synced) == 1                                                     # the device was idle before anything was freed
    assert list(sess.scopes) == ["C", "other", "A", "D"] and "B" not in sess.graphs and ("train_replay", 2) not in sess.graphs
    assert ("propose", "B") not in sess.graphs and {"A", ("propose", "A"), "C", ("propose", "C")} <= set(sess.graphs)
    assert sess.picking and ("train_replay", 1) in sess.graphs                       # A's recording and its running stream search live on
    with sess.shape_scope("E", group="t", cap=2):                                    # a smaller cap drops as many as needed: C and A
        pass
    assert list(sess.scopes) == ["other", "D", "E"] and not sess.picking             # ... and the search that ran on A's recording ended with it
    assert set(sess.graphs) == set()
    assert sess.drop_scope("nope") is False and sess.drop_scope("D") is True


def test_prepared_filter_images_are_session_wide_even_when_first_built_inside_a_scope(sess, monkeypatch):
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: None)
    made = []

    def fn():
        made.append(sess.buf("bwd/wflip/conv", (3, 3)))
        return made[-1]
    with sess.shape_scope("A", group="t", cap=1):
        out = sess.prepared.get(("bwd", "wflip"), fn)
        sess.buf("act", (8,))
    with sess.shape_scope("B", group="t", cap=1):                                    # A is evicted
        pass
    assert "A" not in sess.scopes and out is sess.buffers[("bwd/wflip/conv", (3, 3), torch.float32)]
    assert fn() is out                                                               # what a later refresh() (outside any scope) writes: the same tensor


def test_another_sessions_requests_never_land_in_the_entered_scope(sess):
    """Session B asks for static buffers while A's scope is entered: they are B's (its captured graphs live in B.graphs, which A's eviction
    never drops), and B does not find A's tensors."""
    A, B = sess, _host_session()
    arena = replay.Arena(B, "t")
    with A.shape_scope("k", group="t", cap=2):
        b, h, t = B.buf("act", (8,)), B._store(), arena.take((2, 3), torch.float32, None)
        a = A.buf("act", (8,))
        assert h is B.buffers                                                        # (where h2_buf registers its operand planes)
        assert B.buffers[("act", (8,), torch.float32)] is b and B.buffers[("arena", "t", 0, (2, 3), torch.float32)] is t
        assert A.scopes["k"] == {("act", (8,), torch.float32): a} and a is not b and A._store() is A.scopes["k"]
        assert B.find_buf("act", (8,)) is b and A.find_buf("act", (8,)) is a
        with pytest.raises(KeyError):
            B.find_buf("only_a", A.buf("only_a", (4,)).shape)                        # same name and shape, A's: not B's to find
    assert B.scopes == {} and A.buffers == {} and ops.scope_depth() == 0


def test_h2_operand_planes_follow_the_owner_too(sess, monkeypatch):
    A, B = sess, _host_session()
    monkeypatch.setattr(ops.H2, "empty", staticmethod(lambda rows, K, device: ("planes", rows, K)))
    with A.shape_scope("k", group="t", cap=2):
        assert B.h2_buf("x", 4, 128) is B.buffers[("h2", "x", 4, 128)] and A.h2_buf("x", 4, 128) is A.scopes["k"][("h2", "x", 4, 128)]
    assert ("h2", "x", 4, 128) not in A.buffers and B.scopes == {}


def test_each_session_owns_the_scope_it_entered(sess):
    A, B = sess, _host_session()
    with A.shape_scope("k", group="t", cap=2):
        with B.shape_scope("kb", group="t", cap=2):
            assert ops.scope_depth() == 2
            b, a = B.buf("act", (8,)), A.buf("act", (8,))
            ws = ops.workspace(64, B.device, "x")                                    # scratch follows the innermost entered scope
        a2 = A.buf("act2", (8,))
    assert ops.scope_depth() == 0
    assert B.scopes["kb"] == {("act", (8,), torch.float32): b, ("ws", "cpu", "x", ops.ws_scope): ws} and B.buffers == {}
    assert A.buffers == {("act", (8,), torch.float32): a} and A.scopes["k"] == {("act2", (8,), torch.float32): a2}


def test_an_entered_scope_is_never_evicted(sess):
    with sess.shape_scope("A", group="t", cap=1):
        a = sess.buf("act", (8,))
        with sess.shape_scope("B", group="t", cap=1):                                # over the cap, but A is entered: the group exceeds it
            assert list(sess.scopes) == ["A", "B"] and sess.synced == []
            assert sess.buf("act", (8,)) is not a
            with sess.shape_scope("A", group="t", cap=1):                            # re-entering an entered key: LRU order, nothing else
                assert sess.buf("act", (8,)) is a and list(sess.scopes) == ["B", "A"]
        assert sess.scopes["A"][("act", (8,), torch.float32)] is a and sess.buf("act", (8,)) is a
    assert sess.synced == [] and set(sess.scopes) == {"A", "B"} and ops.scope_depth() == 0
    with sess.shape_scope("C", group="t", cap=1):                                    # nothing entered any more: down to the cap, one synchronize
        assert list(sess.scopes) == ["C"] and len(sess.synced) == 1
    with sess.shape_scope("D", group="t", cap=2):
        with sess.shape_scope("E", group="t", cap=2):                                # the victims are the oldest scopes that are NOT entered
            assert list(sess.scopes) == ["D", "E"] and len(sess.synced) == 2         # (C went, D stayed)


def test_an_exception_leaves_the_scope_stack_where_it_was(sess):
    with sess.shape_scope("A", group="t", cap=2):
        with pytest.raises(ValueError):
            with sess.shape_scope("B", group="t", cap=2):
                raise ValueError("inside a scope")
        assert ops.scope_depth() == 1 and sess._store() is sess.scopes["A"]
        with pytest.raises(ValueError):
            with ops.unscoped():
                assert sess._store() is sess.buffers
                raise ValueError("inside unscoped()")
        assert ops.scope_depth() == 1 and sess._store() is sess.scopes["A"]
    assert ops.scope_depth() == 0


def test_init_host_declares_every_field_the_host_code_reads_on_a_session(sess):
    """runtime.py, replay.py and lib/nets/network.py read these as plain attributes: a misspelt name raises instead of becoming a default."""
    for name in ("variables", "packed", "x3", "h2", "h2_spread", "conv_info", "graphs", "seed", "device_filters_moved", "derived_gen", "device",
                 "buffers", "scopes", "scope_group", "poison_new_buffers", "scope_cap_override", "profile", "flops_last_forward", "flops_by_pipe",
                 "prepared", "picking", "picked_streams", "pick_log"):
        assert name in vars(sess), name
    assert sess.picking is False and sess.picked_streams is None and sess.pick_log == [] and isinstance(sess.graphs, dict)
    assert isinstance(sess.poison_new_buffers, bool) and (sess.scope_cap_override is None or sess.scope_cap_override >= 1)
    assert sess.prepared.device == sess.device and not hasattr(sess, "stream")       # the stream is the GPU part (Session.__init__)
