"""What the four training pieces' wrappers (train_block.py, train_attn.py, train_stem.py, train_heads.py) do alike: pick the
route, say why the kernel route cannot take a set of tensors, allocate the backward's workspace, and give a module an
instance-attribute forward and take it away again.  Every message starts with "route='kernel'" where the kernel route
refuses something: there is no silent fallback.

Needs torch only: a learner does not import the engine."""
import torch


def check_route(route):
    if route not in (None, "kernel", "torch"):
        raise ValueError("route must be 'kernel' or 'torch'")


def resolve(route, lead):
    """`route` as given, or for None "kernel" when `lead` is a CUDA tensor and "torch" otherwise."""
    check_route(route)
    if route is None:
        return "kernel" if isinstance(lead, torch.Tensor) and lead.is_cuda else "torch"
    return route


def tensor_fault(named, device, any_strides=()):
    """The first of `named` - (name, shape, tensor) triples, the shape a tuple - that is not a float32 tensor of that shape
    on `device`, or not contiguous (the names in `any_strides` may have any strides): the reason as a string, or None.
    It runs on every kernel-route call, so it compares `t.shape` as it is and builds nothing."""
    for name, shape, t in named:
        if not isinstance(t, torch.Tensor) or t.shape != shape:
            return "route='kernel' takes %s of shape %s" % (name, list(shape))
        if t.dtype != torch.float32:
            return "route='kernel' needs float32 tensors (%s is %s)" % (name, t.dtype)
        if t.device != device:
            return "route='kernel' needs every tensor on one device (%s is on %s)" % (name, t.device)
        if name not in any_strides and not t.is_contiguous():
            return "route='kernel' needs contiguous tensors (%s is not)" % name
    return None


def cuda_fault(lead):
    return None if lead.is_cuda else "route='kernel' needs CUDA tensors"


def check_knobs(max_workgroups, eps=None):
    """ValueError unless max_workgroups >= 0 and eps (where the piece has one) is finite and positive."""
    if eps is not None and not (eps > 0 and eps != float("inf")):
        raise ValueError("route='kernel' needs a finite eps > 0")
    if max_workgroups < 0:
        raise ValueError("route='kernel' needs max_workgroups >= 0")


def ptr(t):
    return None if t is None else t.data_ptr()


def workspace(bytes_of, n, max_workgroups, device):
    """(uint8 tensor, its size): what the library's `az_train_*_workspace_bytes` asks for a backward of n samples."""
    size = bytes_of(n, max_workgroups)
    return torch.empty(size, dtype=torch.uint8, device=device), size


def adopt(module, flag, forward):
    module.forward = forward                    # an instance attribute: the class's forward stays underneath
    setattr(module, flag, True)


def restore(module, flag):
    """Undoes `adopt`: 1 if the module was adopted under `flag`, else 0."""
    if not module.__dict__.pop(flag, False):
        return 0
    module.__dict__.pop("forward", None)
    return 1
