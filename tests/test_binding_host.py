"""The binding's refusal type, handle owner and decoder forward ladder without a GPU or the shared library: a fake object in
place of `_hip._lib` (put back afterwards)."""
import contextlib
import gc

import pytest
import torch

from gripnet_amd import _hip


class FakeLib:
    """Stands in for the loaded library: writes every call down; `gn_fake_create` hands out handle 77 or fails."""

    def __init__(self, create_status=_hip.GN_OK):
        self.calls, self.create_status = [], create_status

    def gn_last_error(self):
        return b"what the library said"

    def gn_fake_create(self, *args):
        self.calls.append(("create",) + args[:-2])
        if self.create_status == _hip.GN_OK:
            args[-1]._obj.value = 77
        return self.create_status

    def gn_fake_destroy(self, h):
        self.calls.append(("destroy", h.value))


class Owner(_hip.Handle):
    _destroy = "gn_fake_destroy"

    def __init__(self, *args):
        self._create("gn_fake_create", torch.device("cpu"), *args)


@pytest.fixture
def fake(monkeypatch):
    lib = FakeLib()
    monkeypatch.setattr(_hip, "_lib", lib)
    monkeypatch.setattr(_hip, "stream_ptr", lambda device=None: 5)
    monkeypatch.setattr(torch.cuda, "device", lambda device: contextlib.nullcontext())
    return lib


def test_check_maps_every_status_to_its_exception(fake):
    assert _hip.check(_hip.GN_OK) is None
    with pytest.raises(ValueError, match="what the library said"):
        _hip.check(_hip.GN_ERR_INVALID_ARG)
    with pytest.raises(IndexError, match="what the library said"):
        _hip.check(_hip.GN_ERR_INDEX_RANGE)
    with pytest.raises(_hip.Unsupported, match="what the library said") as err:
        _hip.check(_hip.GN_ERR_UNSUPPORTED)
    assert err.value.status == _hip.GN_ERR_UNSUPPORTED == 4
    for status in (_hip.GN_ERR_HIP, _hip.GN_ERR_EDGE_COUNT, 17):
        with pytest.raises(_hip.GripNetHipError, match="what the library said") as err:
            _hip.check(status)
        assert type(err.value) is _hip.GripNetHipError and err.value.status == status
    assert (_hip.GN_ERR_INVALID_ARG, _hip.GN_ERR_INDEX_RANGE) == (1, 3)


def test_a_refusal_is_a_library_error():
    assert issubclass(_hip.Unsupported, _hip.GripNetHipError) and issubclass(_hip.GripNetHipError, RuntimeError)
    assert not issubclass(ValueError, _hip.GripNetHipError) and not issubclass(IndexError, _hip.GripNetHipError)


def test_every_owner_names_its_destroy_entry_point():
    owners = (_hip.GraphPlan, _hip.RgcnPlan, _hip.DistMultPlan, _hip.RelGradPlan, _hip.DistMultBwdPlan, _hip.NegativeSampler,
              _hip.KnownPairs, _hip.MetricsPlan)
    for cls in owners:
        assert issubclass(cls, _hip.Handle) and "__del__" not in vars(cls)
        assert _hip.SIGNATURES[cls._destroy] == (None, [_hip._p])
    assert len({cls._destroy for cls in owners} - {"gn_graph_plan_destroy"}) == 7


def test_a_handle_is_freed_exactly_once(fake):
    owner = Owner(3, 4)
    assert fake.calls == [("create", 3, 4)] and owner._h.value == 77
    owner.__del__()
    assert fake.calls[1:] == [("destroy", 77)] and owner._h is None
    owner.__del__()
    del owner
    gc.collect()
    assert fake.calls[1:] == [("destroy", 77)]


def test_a_dropped_owner_frees_its_handle(fake):
    Owner()
    gc.collect()
    assert fake.calls == [("create",), ("destroy", 77)]


def test_the_stream_and_the_handle_address_end_the_arguments(fake):
    seen = []
    fake.gn_fake_create = lambda *args: seen.append(args) or _hip.GN_OK
    Owner(1, 2)
    assert seen[0][:3] == (1, 2, 5) and isinstance(seen[0][3]._obj, _hip._p) and len(seen[0]) == 4


def test_nothing_is_freed_when_creation_raised(fake):
    fake.create_status = _hip.GN_ERR_UNSUPPORTED
    with pytest.raises(_hip.Unsupported):
        Owner(1)
    fake.create_status = _hip.GN_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        Owner(2)
    gc.collect()
    assert fake.calls == [("create", 1), ("create", 2)]


def test_nothing_is_freed_once_the_library_is_gone(fake, monkeypatch):
    owner = Owner()
    monkeypatch.setattr(_hip, "_lib", None)
    del owner
    gc.collect()
    assert fake.calls == [("create",)]


class FakePlan:
    def __init__(self, error=None):
        self.error, self.calls = error, 0

    def forward(self, z, weight, sigmoid, out):
        self.calls += 1
        if self.error is not None:
            raise self.error
        return out


@pytest.fixture
def plan_less(monkeypatch):
    calls = []
    monkeypatch.setattr(_hip, "distmult_any", lambda z, u_v, edge_type, weight, sigmoid, out: calls.append((u_v, edge_type)) or out)
    return calls


def test_a_plan_that_serves_is_the_only_call(plan_less):
    plan, out = FakePlan(), object()
    assert _hip.distmult_forward("z", "ei", "et", "w", True, out, plan) == (out, True)
    assert plan.calls == 1 and plan_less == []


def test_a_refusing_plan_falls_through_and_says_so(plan_less):
    plan, out = FakePlan(_hip.Unsupported(_hip.GN_ERR_UNSUPPORTED, "node table too large")), object()
    assert _hip.distmult_forward("z", "ei", "et", "w", True, out, plan) == (out, False)
    assert plan.calls == 1 and plan_less == [("ei", "et")]


def test_without_a_plan_the_plan_less_decoder_runs(plan_less):
    out = object()
    assert _hip.distmult_forward("z", "ei", "et", "w", False, out) == (out, False)
    assert plan_less == [("ei", "et")]


@pytest.mark.parametrize("error", [_hip.GripNetHipError(_hip.GN_ERR_HIP, "a HIP error"), ValueError("bad argument"),
                                   IndexError("id out of range")])
def test_any_other_error_of_the_plan_propagates(plan_less, error):
    plan = FakePlan(error)
    with pytest.raises(type(error)) as err:
        _hip.distmult_forward("z", "ei", "et", "w", True, object(), plan)
    assert err.value is error and plan.calls == 1 and plan_less == []
