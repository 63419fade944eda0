"""The routes by which the weights of a `paella_amd.Paella` / `paella_amd.VQModel` change, as one table (test infrastructure; a plain module, not a conftest).

A route is a function `(module, new_sd)` that brings the module to hold exactly the values of `new_sd` (a state dict of fp32 CPU tensors; integer entries as they
are), plus what the contract says about it (`paella_amd.modules._NativeModel._signature`):

  AUTO      the next call serves the new weights with no further call
  REFRESH   the next call serves them after `module.refresh()` only: in-place edits through `.data`, which torch does not version

Every route treats buffers as it treats parameters (a VQModel's BatchNorm statistics are weights of its engine; a Paella has none), reaches the values bit for bit
(the optimizer route takes two exact steps: p - p, then 0 - (-new)), and hands the module tensors of its own: nothing in `new_sd` is aliased or written to.
tests/test_weight_routes.py holds the table against `_signature()` on the CPU, tests/test_gpu_weight_routes.py against a freshly built module on the device.
"""
import collections

import torch
from torch import nn

AUTO, REFRESH = "auto", "refresh"
Route = collections.namedtuple("Route", "name apply contract")


def home(module):
    return next(module.parameters()).device


def other_device(module):
    """a device the module is not on: the CPU for a module on the GPU, the GPU (where there is one) for a module on the CPU; without a GPU the CPU again, which
    still walks the same calls"""
    if home(module).type != "cpu":
        return torch.device("cpu")
    return torch.device("cuda") if torch.cuda.is_available() else torch.device("cpu")


def slots(module):
    """every state-dict entry where it lives: [(key, holder, name, is_buffer)] in state-dict order"""
    out = []
    for prefix, holder in module.named_modules():
        dot = prefix + "." if prefix else ""
        for name, p in holder._parameters.items():
            if p is not None:
                out.append((dot + name, holder, name, False))
        for name, b in holder._buffers.items():
            if b is not None and name not in holder._non_persistent_buffers_set:
                out.append((dot + name, holder, name, True))
    assert [s[0] for s in out] == list(module.state_dict().keys())
    return out


def tensor_of(holder, name, is_buffer):
    return (holder._buffers if is_buffer else holder._parameters)[name]


def _own(module, t, like):
    """`t` as a tensor of the module's own: a copy on its device, in the dtype of the entry it replaces"""
    return t.detach().clone().to(device=like.device, dtype=like.dtype)


def _load(module, sd):
    module.load_state_dict(sd)


def _load_assign(module, sd):
    dev = home(module)
    module.load_state_dict({k: v.detach().clone().to(dev) for k, v in sd.items()}, assign=True)


def _load_from_other_device(module, sd):
    dev = other_device(module)
    module.load_state_dict({k: v.detach().clone().to(dev) for k, v in sd.items()})


@torch.no_grad()
def _inplace(module, sd):
    """ordinary (versioned) in-place ops under no_grad: copy_ on every other entry, zero_ + add_ on the rest"""
    for i, (key, holder, name, is_buffer) in enumerate(slots(module)):
        t = tensor_of(holder, name, is_buffer)
        new = _own(module, sd[key], t)
        if i % 2 == 0 or not t.is_floating_point():
            t.copy_(new)
        else:
            t.zero_().add_(new)


def _sgd(module, sd):
    """two plain SGD steps of lr 1 with gradients set by hand, each exact in fp32: grad = p gives p - p = 0, then grad = -new gives 0 + new; buffers, which no
    optimizer owns, by copy_"""
    named = dict(module.named_parameters())
    opt = torch.optim.SGD(list(named.values()), lr=1.0)
    for step in range(2):
        for key, p in named.items():
            p.grad = p.detach().clone() if step == 0 else -_own(module, sd[key], p)
        opt.step()
    opt.zero_grad(set_to_none=True)
    with torch.no_grad():
        for key, b in module.named_buffers():
            b.copy_(_own(module, sd[key], b))


def _device_round_trip(module, sd):
    """.cpu() then .cuda(), as a checkpoint is loaded on the host and the module moved back: to the other device, load there, and home again"""
    dev = home(module)
    module.to(other_device(module))
    module.load_state_dict(sd)
    module.to(dev)


def _dtype_round_trip(module, sd):
    """.double(), load there, .float(): every fp32 value survives the round trip exactly"""
    module.double()
    module.load_state_dict(sd)
    module.float()


def _data_assign(module, sd):
    for key, holder, name, is_buffer in slots(module):
        t = tensor_of(holder, name, is_buffer)
        t.data = _own(module, sd[key], t)


def _new_objects(module, sd):
    """a NEW Parameter (buffer: tensor) object under every name, by attribute assignment (buffers: register_buffer of a new tensor)"""
    for key, holder, name, is_buffer in slots(module):
        t = tensor_of(holder, name, is_buffer)
        if is_buffer:
            holder.register_buffer(name, _own(module, sd[key], t))
        else:
            setattr(holder, name, nn.Parameter(_own(module, sd[key], t), requires_grad=t.requires_grad))


def _delete_and_register(module, sd):
    for key, holder, name, is_buffer in slots(module):
        t = tensor_of(holder, name, is_buffer)
        new = _own(module, sd[key], t)
        if is_buffer:
            del holder._buffers[name]
            holder.register_buffer(name, new)
        else:
            del holder._parameters[name]
            holder.register_parameter(name, nn.Parameter(new, requires_grad=t.requires_grad))
        del t


def _data_inplace(module, sd):
    """the documented exception: in-place through .data, which bumps no version and moves no pointer"""
    for key, holder, name, is_buffer in slots(module):
        t = tensor_of(holder, name, is_buffer)
        t.data.copy_(_own(module, sd[key], t))


ROUTES = [
    Route("load_state_dict", _load, AUTO),
    Route("load_state_dict_assign", _load_assign, AUTO),
    Route("load_state_dict_other_device", _load_from_other_device, AUTO),
    Route("inplace_no_grad", _inplace, AUTO),
    Route("sgd_step", _sgd, AUTO),
    Route("device_round_trip", _device_round_trip, AUTO),
    Route("dtype_round_trip", _dtype_round_trip, AUTO),
    Route("data_assign", _data_assign, AUTO),
    Route("new_objects", _new_objects, AUTO),
    Route("delete_and_register", _delete_and_register, AUTO),
    Route("data_inplace", _data_inplace, REFRESH),
]
ROUTE_NAMES = [r.name for r in ROUTES]
BY_NAME = {r.name: r for r in ROUTES}


def assert_holds(module, sd):
    """the module's state dict is `sd`, bit for bit, in the module's own dtypes"""
    got = module.state_dict()
    assert sorted(got.keys()) == sorted(sd.keys())
    for k, v in got.items():
        assert v.dtype == sd[k].dtype and torch.equal(v.detach().cpu(), sd[k]), "%s does not hold the new values" % k
