"""What every binding of the package needs to hand torch's tensors to libewn_hip.so, and nothing about any one of them: pointers and
the stream, the descriptions and checks of buffers and inputs, the checks of plain numbers.  Imports _lib and no other module of the
package."""
import ctypes as C
import math

import numpy as np
import torch

from . import _lib


def _require_gpu(device):
    if not torch.cuda.is_available():
        raise _lib.EwnError("ewn_gym_amd needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU fallback")
    return torch.device(device)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _describe(t):
    if not isinstance(t, torch.Tensor):
        return type(t).__name__
    return "%s %s on %s%s" % (t.dtype, list(t.shape), t.device, "" if t.is_contiguous() else " (not contiguous)")


def _is_buffer(t, dtype):
    return isinstance(t, torch.Tensor) and t.dtype == dtype and t.is_cuda and t.is_contiguous()


def _check_buffer(who, name, t, dtype, lead, shape):
    """ValueError unless t is a contiguous device tensor of `dtype` and shape [>= lead, *shape] (lead None: exactly `shape`)"""
    if not (_is_buffer(t, dtype) and (tuple(t.shape) == shape if lead is None else
                                      t.dim() == 1 + len(shape) and t.shape[0] >= lead and tuple(t.shape[1:]) == shape)):
        dims = ([] if lead is None else [">= %d" % lead]) + [str(x) for x in shape]
        raise ValueError("%s: %s must be a contiguous %s device tensor of shape [%s], got %s" % (
            who, name, str(dtype).replace("torch.", ""), ", ".join(dims), _describe(t)))


def _policy_input(name, x, dtype, shape, dev, who="predict_policy"):
    """a tensor is taken as it is and must already be what the kernel reads; anything else (numpy, lists) is copied to the device"""
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.asarray(x)).to(dtype).reshape(shape)
        return x if dev.type != "cuda" else x.to(dev)
    if x.dtype != dtype or x.numel() != math.prod(shape) or not x.is_contiguous():
        raise ValueError("%s: %s must be a contiguous %s tensor of %s elements, got %s" % (
            who, name, str(dtype).replace("torch.", ""), " x ".join(map(str, shape)), _describe(x)))
    return x.reshape(shape)


def _obs_ids(obs_id, dev):
    """host obs_id (numbers 0 .. 2^32 - 1, or None) -> the int32 tensor on dev that the kernels read: a copy, the uint32 bit patterns"""
    if obs_id is None:
        return None
    return torch.from_numpy(np.asarray(obs_id, dtype=np.uint32).reshape(-1).view(np.int32).copy()).to(dev)


def _lookahead_shape(who, boards, cube_layer=None):
    """(M, S, P) of boards [S, S] or [M, S, S], P the policy network's parameter count; ValueError where there is no policy network for
    the geometry.  cube_layer None: any board size, P None"""
    shp = tuple(boards.shape) if isinstance(boards, torch.Tensor) else np.asarray(boards).shape
    if len(shp) == 2:
        shp = (1,) + tuple(shp)
    if len(shp) != 3 or shp[1] != shp[2]:
        raise ValueError("%s: boards must have shape [S, S] or [M, S, S], got %s" % (who, list(shp)))
    M, S = int(shp[0]), int(shp[1])
    P = None if cube_layer is None else _lib.load().ewn_policy_param_count(S, int(cube_layer))
    if P is not None and P < 0:
        raise ValueError("%s: no policy network for %dx%d boards with cube_layer %d (served: cube_layer 3 on 5x5 and 7x7)" % (
            who, S, S, cube_layer))
    return M, S, P


def _policy_params(who, params, P, S):
    """params is the flat fp32 vector of the SxS actor-critic, P elements -> its device, where everything else has to live"""
    if not (isinstance(params, torch.Tensor) and params.dtype == torch.float32 and params.is_contiguous() and params.numel() == P):
        raise ValueError("%s: params must be a contiguous float32 tensor of %d elements (the %dx%d actor-critic), got %s" % (
            who, P, S, S, _describe(params)))
    return params.device


def _same_gpu(who, dev, holder, named):
    """every tensor of named = [(name, tensor or None)] lives on dev, a GPU: the one that holds `holder`"""
    for name, t in named:
        if t is not None and not (t.is_cuda and t.device == dev):
            raise ValueError("%s: %s must live on the GPU that holds %s (%s), got %s" % (who, name, holder, dev, _describe(t)))


# ---------------------------------------------------------------- plain numbers: each returns the checked value

def _finite(who, name, v):
    if not math.isfinite(float(v)):
        raise ValueError("%s: %s must be finite, got %r" % (who, name, v))
    return float(v)


def _not_negative(who, name, v):
    if not math.isfinite(float(v)) or float(v) < 0.0:
        raise ValueError("%s: %s must be finite and not negative, got %r" % (who, name, v))
    return float(v)


def _positive(who, name, v):
    if not math.isfinite(float(v)) or not float(v) > 0.0:
        raise ValueError("%s: %s must be finite and positive, got %r" % (who, name, v))
    return float(v)


def _at_least_one(who, name, v):
    if int(v) < 1:
        raise ValueError("%s: %s must be at least 1, got %r" % (who, name, v))
    return int(v)
