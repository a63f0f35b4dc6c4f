"""ctypes binding of libpdfnet_hip.so -- the drop-in C-ABI boundary (include/pdfnet_hip.h).

The product path has NO fallback: if the library is missing, import fails loudly; if a call returns
non-zero, a RuntimeError is raised (the reference's only native op calls exit(-1) on a launch error,
lib/utils/roi_align/src/cuda/crop_and_resize_kernel.cu:186-191 -- we raise instead).
torch is used only for device memory (tensor.data_ptr()) and the current HIP stream handle.
"""
import ctypes
import os
import re

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PDFNET_HIP_LIB") or os.path.join(_HERE, "libpdfnet_hip.so")   # override: A/B of two builds in one session
HEADER_PATH = os.path.join(_HERE, "..", "include", "pdfnet_hip.h")

_CT = {"int": ctypes.c_int, "long": ctypes.c_long, "float": ctypes.c_float,
       "unsigned long long": ctypes.c_ulonglong}


def _text(path):
    return re.sub(r"/\*.*?\*/", "", open(path).read(), flags=re.S)


def parse_header(path=HEADER_PATH):
    """-> {name: (restype, [argtypes])} for every `int|long pdf_*(...)` prototype in the header."""
    protos = {}
    for m in re.finditer(r"\b(int|long)\s+(pdf_\w+)\s*\(([^)]*)\)\s*;", _text(path)):
        ret, name, args = m.group(1), m.group(2), m.group(3)
        types = []
        for a in args.split(","):
            a = " ".join(a.split())
            if a in ("", "void"):
                continue
            if "*" in a:
                types.append(ctypes.c_void_p)
            else:
                base = a.rsplit(" ", 1)[0]
                types.append(_CT[base])
        protos[name] = (_CT[ret], types)
    return protos


def parse_structs(path=HEADER_PATH):
    """-> {name: ctypes.Structure class} for every `typedef struct Name { ... } Name;` of the header, in its order and with its field names.
    Fields: a pointer (void* here), int / long / float / unsigned long long, an earlier struct; `a, b` declarator lists and `[n]` arrays.
    Anything else raises: a layout is never guessed."""
    txt, structs = _text(path), {}
    for m in re.finditer(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;", txt):
        fields = []
        for decl in filter(None, (" ".join(d.split()) for d in m.group(2).split(";"))):
            try:
                first, *more = decl.split(",")
                base, star, name, dim = re.fullmatch(r"(?:const )?([\w ]+?) ?(\*?) ?(\w+)(?:\[(\d+)\])?", first).groups()
                ct = ctypes.c_void_p if star else _CT.get(base) or structs[base]
                names = [(name, dim)] + [re.fullmatch(r" ?(\w+)(?:\[(\d+)\])?", d).groups() for d in more]
                if star and more:                    # `float* a, b`: b is no pointer -- not written in this header, not bound
                    raise KeyError(decl)
            except (AttributeError, KeyError):       # no match / unknown type
                raise ImportError("pdfnet_amd: %s: cannot bind field `%s` of %s" % (path, decl, m.group(1)))
            fields += [(n, ct * int(d) if d else ct) for n, d in names]
        structs[m.group(1)] = type(m.group(1), (ctypes.Structure,), {"_fields_": fields})
    if len(structs) != len(re.findall(r"\b(?:struct|union)\b[^;(]*\{", txt)):
        raise ImportError("pdfnet_amd: %s has a struct / union this binding cannot parse" % path)
    return structs


STRUCTS = parse_structs()          # built once at import; a call only fills fields
CallOpts, MeshLevel, MeshLoss = (STRUCTS[n] for n in ("PdfCallOpts", "PdfMeshLevel", "PdfMeshLoss"))


class _Lib:
    def __init__(self):
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "pdfnet_amd: %s is missing -- build it with `python -m pdfnet_amd.build` "
                "(hipcc --offload-arch=gfx950). There is no CPU or PyTorch fallback." % LIB_PATH)
        self.cdll = ctypes.CDLL(LIB_PATH)
        self.protos = parse_header()
        for name, (ret, args) in self.protos.items():
            fn = getattr(self.cdll, name)          # AttributeError if the .so does not export it
            fn.restype = ret
            fn.argtypes = args
        for cls, fn in ((CallOpts, "pdf_debug_callopts_size"), (MeshLoss, "pdf_debug_mesh_loss_size"), (MeshLevel, "pdf_debug_mesh_level_size")):
            if getattr(self.cdll, fn)() != ctypes.sizeof(cls):
                raise ImportError("pdfnet_amd: %s of %s has %d bytes, this binding's has %d -- rebuild the library"
                                  % (cls.__name__, LIB_PATH, getattr(self.cdll, fn)(), ctypes.sizeof(cls)))

    def __getattr__(self, name):
        fn = getattr(self.cdll, name)
        is_status = self.protos[name][0] is ctypes.c_int and not name.startswith("pdf_debug_")     # int = status code

        def call(*args):
            rc = fn(*args)
            if is_status and rc != 0:
                raise RuntimeError("libpdfnet_hip: %s failed with code %d" % (name, rc))
            if _tape is not None and is_status:                # (taped.TapedSegment is recording: launches only, not size queries)
                _tape.append((call, args))
            return rc
        setattr(self, name, call)
        return call


_lib = None
_tape = None            # a list while pdfnet_amd.taped records a segment: every status-returning library call is appended as (callable, args)


def lib():
    global _lib
    if _lib is None:
        _lib = _Lib()
        if torch.cuda.is_available():
            # The library's rings live on the device that is current NOW (one process = one GPU).  Under a multi-GPU
            # launcher the rank must have selected its GPU first: binding the library before
            # torch.cuda.set_device(LOCAL_RANK) would put every rank's rings on GPU 0.
            lr = os.environ.get("LOCAL_RANK")
            if lr is not None and torch.cuda.device_count() > 1 and int(lr) != torch.cuda.current_device():
                _lib = None
                raise RuntimeError("pdfnet_amd: LOCAL_RANK=%s but the current device is cuda:%d -- call torch.cuda.set_device(LOCAL_RANK) "
                                   "(trains.base_trainer.init_distributed) before the first pdfnet_amd call" % (lr, torch.cuda.current_device()))
            _lib.pdf_init()                # device-side ticket counters: allocate now, never inside a stream capture
    return _lib


def check_device(dev):
    """Raise if tensors on `dev` would be handed to a library whose rings live on another GPU."""
    L = lib()
    have = L.pdf_debug_init_device()
    idx = dev.index if dev.index is not None else torch.cuda.current_device()
    if have >= 0 and have != idx:
        raise RuntimeError("pdfnet_amd: libpdfnet_hip was initialised on cuda:%d, the model lives on cuda:%d (one process per GPU)" % (have, idx))


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_raw_device = getattr(torch._C, "_cuda_getDevice", None)


def stream():
    """hipStream_t of torch's current stream (launches are captured when that stream is capturing).
    Called once per kernel launch (~2,000 times a step): the raw-handle query costs ~0.3 us where
    `torch.cuda.current_stream()` builds a Stream object through the device-index helpers (~9 us, a fifth of the step's
    host time)."""
    if _raw_stream is not None and _raw_device is not None:
        return _raw_stream(_raw_device())
    return torch.cuda.current_stream().cuda_stream


def ptr(t):
    """Device address as a plain int (ctypes converts ints and None for `void*` parameters itself; ~7,000 pointers a step)."""
    return t.data_ptr() if t is not None else None


def ptr_at(t, elements):
    """Device pointer `elements` elements into `t` (a channel offset inside an NHWC row)."""
    return t.data_ptr() + elements * t.element_size()


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError("pdfnet_amd ops run only on the GPU (HIP); got a %s tensor. "
                               "There is no CPU fallback in the product path." % t.device)
