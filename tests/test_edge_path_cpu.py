"""gnn.EdgePath on the host: the edge stage's settings, the scaled stage's
exponents and the guard's table of per-pass flags.  The object is built on
torch.device('cpu'), so the table is a host tensor and a test raises a flag by
indexing it, as a kernel would with its atomic OR."""
import threading

import pytest
import torch

import pointgnn_amd  # noqa: F401
from pointgnn_amd import gnn

ROWS, SLOTS = gnn.EDGE_SCALE_ROWS, gnn.EDGE_SCALE_SLOTS
RANGE = SLOTS        # the range flag's column: behind the scaled layers'


def edge_path(**kw):
    return gnn.EdgePath(device=torch.device("cpu"), **kw)


def cell(edge, address):
    """(row, column) of a status address in the table."""
    words, rest = divmod(address - edge.flags.data_ptr(), 4)
    assert rest == 0 and 0 <= words < edge.flags.numel()
    return divmod(words, edge.flags.shape[1])


def test_rows_are_handed_out_round_robin():
    edge = edge_path()
    rows = [edge.take_row() for _ in range(2 * ROWS + 3)]
    assert sorted(set(rows)) == list(range(ROWS))
    for a, b in zip(rows, rows[1:]):
        assert b == (a + 1) % ROWS
    assert edge.row == rows[-1]


def test_each_thread_sees_the_row_it_took():
    edge = edge_path()
    both_took = threading.Barrier(2)
    seen = {}
    mine = edge.row

    def work(name):
        took = edge.take_row()
        both_took.wait(timeout=10)      # (the other thread has taken its own)
        seen[name] = (took, edge.row, cell(edge, edge.status('range'))[0])
    threads = [threading.Thread(target=work, args=(n,)) for n in "ab"]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert seen["a"][0] != seen["b"][0]
    for took, current, pointed_at in seen.values():
        assert took == current == pointed_at
    assert edge.row == mine     # this thread took none


def test_slots_in_first_use_order_and_their_limit():
    edge = edge_path()
    assert edge.flags is None
    row = edge.take_row()
    assert edge.flags is None       # (made by the first status request)
    scopes = ["layer%d" % i for i in range(SLOTS)]
    for i, s in enumerate(scopes):
        assert cell(edge, edge.status('scale', s)) == (row, i)
    assert tuple(edge.flags.shape) == (ROWS, SLOTS + 1)
    assert edge.flags.dtype == torch.int32 and not edge.flags.any()
    # asked again, in another order: the same columns
    for i, s in reversed(list(enumerate(scopes))):
        assert cell(edge, edge.status('scale', s)) == (row, i)
    assert edge.slots == {s: i for i, s in enumerate(scopes)}
    with pytest.raises(NotImplementedError):
        edge.status('scale', "layer%d" % SLOTS)
    # the range flag's column is none of theirs
    assert cell(edge, edge.status('range')) == (row, RANGE)
    assert RANGE not in edge.slots.values()


def test_verdict_reports_range_and_scale_separately_and_clears_its_rows():
    edge = edge_path(arith='f16x2')
    edge.exps.update(a=3, b=5)
    r, other = edge.take_row(), edge.take_row()
    col = {s: cell(edge, edge.status('scale', s))[1] for s in "ab"}
    edge.status('range')
    assert edge.read([r]) == gnn.EdgeVerdict(False, False)
    edge.flags[r, RANGE] = 1
    edge.flags[other, col["a"]] = 1
    assert edge.read([r]) == gnn.EdgeVerdict(True, False)
    assert not edge.flags[r].any() and edge.flags[other, col["a"]] == 1
    assert edge.exps == dict(a=3, b=5)
    edge.flags[r, col["b"]] = 1
    assert edge.read([r]) == gnn.EdgeVerdict(False, True)
    assert not edge.flags[r].any() and edge.flags[other, col["a"]] == 1
    assert edge.exps == dict(a=3, b=7)      # the tripped layer's alone
    # asked about scale flags only: a range flag stays for whoever asks
    edge.flags[r, RANGE] = 1
    edge.flags[r, col["a"]] = 1
    assert edge.read([r], kinds=('scale',)) == gnn.EdgeVerdict(False, True)
    assert edge.flags[r].tolist() == [0] * SLOTS + [1]
    assert edge.read(kinds=('range',)) == gnn.EdgeVerdict(True, False)
    assert edge.flags[other, col["a"]] == 1 and not edge.flags[r].any()
    # host values the caller read itself
    values = edge.flags[other].tolist()
    assert edge.verdict({other: values}) == gnn.EdgeVerdict(False, True)
    assert not edge.flags.any()
    assert edge.exps == dict(a=7, b=7)


def test_exponents_rise_by_two_up_to_24_and_only_when_counted():
    edge = edge_path()
    edge.exps.update(a=21, b=4)
    r = edge.take_row()
    col = {s: cell(edge, edge.status('scale', s))[1] for s in "ab"}
    for want in (23, 24, 24):
        edge.flags[r, col["a"]] = 1
        assert edge.read([r]).scale
        assert edge.exps == dict(a=want, b=4)
    edge.flags[r, col["b"]] = 1
    assert edge.read([r], count=False).scale
    assert edge.exps == dict(a=24, b=4) and not edge.flags.any()
    edge.flags[r, col["b"]] = 1
    edge.discard(r)
    assert edge.exps == dict(a=24, b=4) and not edge.flags.any()
    assert not edge.read([r]).scale


def test_plain_path_and_back():
    edge = edge_path(arith='f16x2', scaled=True)
    with edge.plain():
        assert (edge.arith, edge.scaled) == ('f32', False)
    assert (edge.arith, edge.scaled) == ('f16x2', True)
    edge.arith = 'bf16x3'
    with edge.plain():
        assert (edge.arith, edge.scaled) == ('bf16x3', False)
    assert (edge.arith, edge.scaled) == ('bf16x3', True)
    edge.arith = 'f16x2'
    with pytest.raises(KeyError):
        with edge.plain():
            assert (edge.arith, edge.scaled) == ('f32', False)
            raise KeyError("from the body")
    assert (edge.arith, edge.scaled) == ('f16x2', True)
    with pytest.raises(ValueError):
        edge.arith = 'f8'
    assert edge.arith == 'f16x2'


def test_settings_outlive_new_weights_and_the_rest_does_not():
    edge = edge_path(arith='bf16x3', scaled=True, k300=False)
    edge.take_row()
    edge.status('scale', "a")
    edge.exps["a"] = 6
    store = gnn.ParamStore({}, torch.device("cpu"), edge)
    assert store.edge is edge
    assert (edge.arith, edge.scaled, edge.k300) == ('bf16x3', True, False)
    assert edge.exps == {} and edge.slots == {} and edge.flags is None
    bare = gnn.ParamStore({}).edge
    assert (bare.arith, bare.scaled, bare.flags) == ('f32', False, None)


@pytest.mark.parametrize("max_abs,want", [
    (0.0, 0), (gnn.EDGE_SCALE_HEADROOM, 0),
    (gnn.EDGE_SCALE_HEADROOM * (1 + 2.0 ** -20), 1), (float("inf"), 24),
    (float("nan"), 24)])
def test_exponent_for_a_maximum(max_abs, want):
    assert gnn.edge_scale_exp_for(max_abs) == want
