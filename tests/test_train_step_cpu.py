"""Which step engine a Trainer runs and when an engine's weight images are
refreshed (pointgnn_amd.train_step.StepSelector / StepEngine), with two fake
engines that record their calls.  No GPU: the rules are host logic."""
import pytest

import pointgnn_amd  # noqa: F401
from pointgnn_amd.train_step import StepEngine, StepSelector

BATCH = ("input_v", "coords", "kps", "edges")


class FakeEngine(StepEngine):
    def __init__(self, name, log, stale):
        self.name, self.log, self._stale = name, log, stale

    def _repack(self):
        self.log.append((self.name, "repack"))

    def _forward(self, *batch):
        assert batch == BATCH
        self.log.append((self.name, "forward"))
        return "logits", "pred", self.name + "-state"

    def backward(self, state, dlogits, dpred, sync_sums=None):
        self.log.append((self.name, "backward", state))
        return self.name == "native"


class Holder(StepSelector):
    """What Trainer.__init__ sets up: no native engine yet, the composed
    engine's images not built, one repack()."""

    def __init__(self, native_available=True):
        self.log = []
        self.native, self.sparse_adjoint = True, True
        self.native_available = native_available
        self._native_step = None
        self._composed_step = FakeEngine("composed", self.log, stale=True)
        self._saved = None
        self.created = 0
        self.repack()

    def _create_native_step(self):
        self.created += 1
        if not self.native_available:
            return None
        # (a created handle packs its images when it binds)
        return FakeEngine("native", self.log, stale=False)

    def calls(self, name, what):
        return sum(e[:2] == (name, what) for e in self.log)


@pytest.mark.parametrize("native,sparse,want", [
    (True, True, "native"), (True, False, "composed"),
    (False, True, "composed"), (False, False, "composed")])
def test_engine_of_each_setting(native, sparse, want):
    h = Holder()
    assert h.log == []             # nothing to repack before the first forward
    h.native, h.sparse_adjoint = native, sparse
    assert h._engine().name == want
    assert (h._native_step is not None) == (want == "native")
    assert h.forward(*BATCH) == ("logits", "pred")
    assert [e for e in h.log if e[1] == "forward"] == [(want, "forward")]
    # the flags are the caller's: selecting does not change them
    assert (h.native, h.sparse_adjoint) == (native, sparse)
    assert h.created == (1 if want == "native" else 0)


@pytest.mark.parametrize("first", ["native", "composed"])
def test_repack_refreshes_the_engine_in_use_and_the_other_lazily(first):
    other = "composed" if first == "native" else "native"
    h = Holder()
    for name in (other, first):      # both engines exist, `first` is selected
        h.native = name == "native"
        h.forward(*BATCH)
    del h.log[:]
    h.repack()                       # (an optimizer step was applied)
    assert h.log == [(first, "repack")]
    h.forward(*BATCH)                # the selected engine: already fresh
    assert h.log == [(first, "repack"), (first, "forward")]
    del h.log[:]
    h.native = other == "native"
    h.forward(*BATCH)
    h.forward(*BATCH)
    assert h.log == [(other, "repack"), (other, "forward"),
                     (other, "forward")]


def test_backward_goes_to_the_engine_of_the_last_forward():
    h = Holder()
    h.forward(*BATCH)
    h.native = False
    assert h.backward("dlogits", "dpred", "sums") is True
    assert h.log[-1] == ("native", "backward", "native-state")
    assert h._saved is None
    h.forward(*BATCH)
    h.native = True
    assert h.backward("dlogits", "dpred") is False
    assert h.log[-1] == ("composed", "backward", "composed-state")
    assert h.calls("native", "backward") == h.calls("composed", "backward") == 1


def test_a_model_without_a_native_step_runs_composed_in_the_same_call():
    h = Holder(native_available=False)
    assert h.native and h.log == []
    assert h.forward(*BATCH) == ("logits", "pred")
    assert h.native is False and h._native_step is None
    assert h.log == [("composed", "repack"), ("composed", "forward")]
    assert h._saved == (h._composed_step, "composed-state")
    h.forward(*BATCH)
    assert h.created == 1            # not asked for again while native is off
    assert h.calls("composed", "forward") == 2
    assert h.calls("composed", "repack") == 1
