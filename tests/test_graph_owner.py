"""CPU: the owner protocol of a captured graph (`paella_amd._graph.GraphOwner`) on a stub, and the input staging of `GraphSampler` / `GraphInpainter`, which
accepts every input of a call before it copies any.  Nothing here touches a device: the stub's capture only counts, and the samplers are built without one.
What the real owners capture and replay is tests/test_gpu_graph.py's, test_gpu_request_stream.py's and test_gpu_train_graph.py's."""
import pytest
import torch

from paella_amd._graph import GraphOwner
from paella_amd.editing import GraphInpainter
from paella_amd.sampling import GraphSampler


class _Stub(GraphOwner):
    """an owner whose capture only counts and whose state is a list the test mutates"""

    _stale_hint = "edit the list"

    def __init__(self, state, on_stale="recapture"):
        self._init_owner(on_stale)
        self.state, self.veto = state, None
        self._capture()

    def _state(self):
        return [tuple(e) for e in self.state]

    def _capture(self):
        self.graph, self._captured_state = object(), self._state()
        self.captures += 1

    def _refuse_recapture(self, causes):
        if self.veto is not None:
            raise RuntimeError("%s: %s" % (self.veto, ", ".join(causes)))


def test_on_stale_is_validated_at_construction():
    for bad in ("ignore", None, "Raise", ""):
        with pytest.raises(ValueError, match="on_stale must be 'recapture' or 'raise'"):
            _Stub([["weights", 1]], on_stale=bad)
    assert _Stub([["weights", 1]], on_stale="raise").on_stale == "raise" and _Stub([["weights", 1]]).on_stale == "recapture"


@pytest.mark.parametrize("on_stale", ["recapture", "raise"])
def test_fresh_state_is_left_alone(on_stale):
    o = _Stub([["weights", 1], ["precision", 0]], on_stale=on_stale)
    assert o.captures == 1 and o._stale() == []
    graph = o.graph
    for _ in range(3):
        o._check_fresh()
    assert o.captures == 1 and o.graph is graph


def test_a_changed_entry_is_named():
    o = _Stub([["weights", 1], ["precision", 0], ["train mode", True]])
    o.state[1][1] = 1
    assert o._stale() == ["precision"]
    o.state[2][1] = False
    assert o._stale() == ["precision", "train mode"]
    o.state[1][1] = 0
    assert o._stale() == ["train mode"]


def test_raise_names_the_causes_and_keeps_the_capture():
    o = _Stub([["weights", 1], ["precision", 0], ["train mode", True]], on_stale="raise")
    graph = o.graph
    o.state[0][1] = 2
    o.state[2][1] = False
    for _ in range(2):          # refusing does not make it fresh
        with pytest.raises(RuntimeError) as e:
            o._check_fresh()
        text = str(e.value)
        assert "stale" in text and "weights, train mode" in text and "precision" not in text
        assert text.startswith("_Stub: the captured graph is stale") and "(edit the list)" in text and "Build a new _Stub" in text and "on_stale='recapture'" in text
    assert o.captures == 1 and o.graph is graph
    o.state[0][1] = 1
    o.state[2][1] = True
    o._check_fresh()            # back to what the capture saw: fresh again
    assert o.captures == 1


def test_recapture_captures_once_and_is_then_fresh():
    o = _Stub([["weights", 1], ["precision", 0]])
    graph = o.graph
    o.state[0][1] = 2
    o._check_fresh()
    assert o.captures == 2 and o.graph is not graph and o._stale() == []
    o._check_fresh()
    assert o.captures == 2


@pytest.mark.parametrize("on_stale", ["recapture", "raise"])
def test_the_veto_comes_ahead_of_both(on_stale):
    o = _Stub([["weights", 1], ["precision", 0]], on_stale=on_stale)
    o.veto = "busy"
    o._check_fresh()            # fresh: the veto is not asked
    o.state[1][1] = 1
    with pytest.raises(RuntimeError, match="^busy: precision$"):
        o._check_fresh()
    assert o.captures == 1 and o._stale() == ["precision"]


def test_the_noun_and_the_hint_are_the_class_s():
    class Step(_Stub):
        _noun, _stale_hint = "captured iteration", ""
    o = Step([["train mode", True]], on_stale="raise")
    o.state[0][1] = False
    with pytest.raises(RuntimeError, match=r"^Step: the captured iteration is stale -- changed since the capture: train mode\.  Build a new Step or"):
        o._check_fresh()


# ---------------------------------------------------------------------------------------------------------------------
# GraphSampler input staging: a refused replay leaves the capture's buffers as they were
# ---------------------------------------------------------------------------------------------------------------------
def _cond(seed, images=2):
    g = torch.Generator().manual_seed(seed)
    return {"byt5": torch.randn(2, 3, 8, generator=g), "clip": torch.randn(2, 4, generator=g),
            "clip_image": [torch.randn(2, 4, generator=g) for _ in range(images)] if images else None}


def _sampler(cls=GraphSampler, uncond_images=0):
    """a sampler without a capture: the static input buffers alone, a freshness check that finds nothing, no device words and a replay that does nothing"""
    s = object.__new__(cls)
    s.cond, s.uncond = _cond(1), _cond(2, images=uncond_images)
    s._check_fresh = lambda: None
    s._set_words = lambda seed, shard: None
    s.graph, s.out = type("NoGraph", (), {"replay": lambda self: None})(), None
    return s


def _buffers(s):
    out = [getattr(s, n) for n in ("images", "mask") if hasattr(s, n)]
    for d in (s.cond, s.uncond):
        for v in ({} if d is None else d).values():
            out += [] if v is None else list(v) if isinstance(v, list) else [v]
    return out


def _refused(s, match, *args):
    """the replay raises ValueError and every destination tensor is bit-equal to what it was (and still the same object)"""
    held = _buffers(s)
    before = [t.clone() for t in held]
    with pytest.raises(ValueError, match=match):
        s(*args)
    now = _buffers(s)
    assert len(now) == len(held) and all(a is b for a, b in zip(now, held))
    assert all(torch.equal(a, b) for a, b in zip(held, before))


def test_accepted_inputs_are_copied_and_none_keeps():
    s = _sampler()
    new_c, new_u = _cond(11), _cond(12, images=0)
    keep_u = [t.clone() for t in _buffers(s)[4:]]
    s(new_c, None)
    assert torch.equal(s.cond["byt5"], new_c["byt5"]) and torch.equal(s.cond["clip"], new_c["clip"])
    assert all(torch.equal(a, b) for a, b in zip(s.cond["clip_image"], new_c["clip_image"]))
    assert all(torch.equal(a, b) for a, b in zip(_buffers(s)[4:], keep_u))
    s(None, new_u)
    assert torch.equal(s.uncond["byt5"], new_u["byt5"]) and torch.equal(s.uncond["clip"], new_u["clip"]) and torch.equal(s.cond["byt5"], new_c["byt5"])


def test_one_wrong_shape_among_good_keys_copies_nothing():
    s = _sampler()
    for key in ("byt5", "clip"):            # the first key and one behind a good one
        bad = _cond(11)
        bad[key] = torch.zeros(2, 5, 8) if key == "byt5" else torch.zeros(2, 5)
        _refused(s, r"conditioning shape differs from the captured one \(%s\)" % key, bad, None)
    bad = _cond(11)
    bad["clip_image"][1] = torch.zeros(2, 5)  # the last tensor of the last key
    _refused(s, r"conditioning layout differs from the captured one \(clip_image: list length / shapes\)", bad, None)


def test_a_list_of_the_wrong_length_copies_nothing():
    s = _sampler()
    _refused(s, r"clip_image: list length / shapes", _cond(11, images=3), None)
    _refused(s, r"clip_image: list length / shapes", _cond(11, images=1), None)
    one = _cond(11)
    one["clip_image"] = one["clip_image"][0]  # a tensor where the capture holds a list
    _refused(s, r"clip_image: list length / shapes", one, None)


def test_a_key_the_capture_had_none_for_copies_nothing():
    s = _sampler()
    _refused(s, r"conditioning layout differs from the captured one \(clip_image\)", None, _cond(12, images=1))
    s.uncond = None
    _refused(s, "captured without this conditioning set", _cond(11), _cond(12))


def test_a_bad_unconditional_set_behind_a_good_conditional_one_copies_nothing():
    s = _sampler()
    bad_u = _cond(12, images=0)
    bad_u["clip"] = torch.zeros(3, 4)
    _refused(s, r"conditioning shape differs from the captured one \(clip\)", _cond(11), bad_u)
    missing = _cond(12, images=0)
    missing["byt5"] = None
    _refused(s, r"conditioning shape differs from the captured one \(byt5\)", _cond(11), missing)


def test_inpainter_stages_images_mask_and_conditioning_together():
    s = _sampler(GraphInpainter)
    s.images, s.mask = torch.rand(2, 3, 16, 16), torch.ones(2, 2, 2, dtype=torch.int64)
    good_i, good_m = torch.rand(2, 3, 16, 16), torch.zeros(2, 2, 2, dtype=torch.int64)
    _refused(s, "mask shape differs from the captured one", good_i, torch.zeros(2, 4, 4, dtype=torch.int64), _cond(11), None)
    _refused(s, "image shape differs from the captured one", torch.rand(2, 3, 8, 8), good_m, _cond(11), None)
    bad_u = _cond(12, images=0)
    bad_u["byt5"] = torch.zeros(2, 9, 8)
    _refused(s, r"conditioning shape differs from the captured one \(byt5\)", good_i, good_m, _cond(11), bad_u)
    s(good_i, None)
    assert torch.equal(s.images, good_i) and bool((s.mask == 1).all())
