"""ctypes binding of libvllm_hip.so.  The header ``include/vllm_hip.h`` is the single source of truth: the prototypes AND the
descriptor structs (``_lib.VllmVitDesc``, ...) are parsed from it (and from ``include/vllm_hip_gdino_encoder.h`` and
``include/vllm_hip_gdino_inputs.h``, which it includes for the descriptors of its sections f2g and f2h) when this module is imported,
which does not load the library.
Loading it (``lib()``) fails when a declared symbol is not exported, and checks every struct's size against the library's own
``vllm_*_sizeof()`` once."""
import ctypes
import os
import re
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
_ROOT = os.path.dirname(_HERE)
HEADER = os.path.join(_ROOT, "include", "vllm_hip.h")
GDINO_ENCODER_HEADER = os.path.join(_ROOT, "include", "vllm_hip_gdino_encoder.h")   # section f2g's descriptors; vllm_hip.h includes it
GDINO_INPUTS_HEADER = os.path.join(_ROOT, "include", "vllm_hip_gdino_inputs.h")     # section f2h's descriptor; vllm_hip.h includes it

_lib = None

_CTYPES = {
    "int": ctypes.c_int, "long": ctypes.c_long, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
    "double": ctypes.c_double, "vllm_stream_t": ctypes.c_void_p, "size_t": ctypes.c_size_t,
}


def lib_path() -> str:
    """In-tree build; VLLM_HIP_LIB names another build of the same ABI (A/B timing of two builds in one session)."""
    return os.environ.get("VLLM_HIP_LIB") or os.path.join(_HERE, "_build", "libvllm_hip.so")


def build(force: bool = False, jobs: int = 8) -> str:
    """Compile every HIP source for gfx950 (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-s", "-C", os.path.join(_HERE, "csrc"), f"-j{jobs}"]
    if force:
        cmd.append("-B")
    subprocess.check_call(cmd)
    return lib_path()


def parse_header(path: str = HEADER):
    """-> {name: (restype, [argtypes])} for every ``vllm_*`` function declared in the header."""
    src = open(path).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    protos = {}
    for m in re.finditer(r"\b(int|long|void|const\s+char\s*\*)\s*(vllm_\w+)\s*\(([^)]*)\)\s*;", src):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        restype = (ctypes.c_char_p if "char" in ret else None if ret == "void"
                   else ctypes.c_long if ret == "long" else ctypes.c_int)
        argtypes = []
        if args and args != "void":
            for a in args.split(","):
                a = a.strip()
                if "char" in a and "*" in a:
                    argtypes.append(ctypes.c_char_p)
                elif "*" in a:
                    argtypes.append(ctypes.c_void_p)
                else:
                    toks = [t for t in a.replace("const", " ").split() if t]
                    argtypes.append(_CTYPES[toks[0]])
        protos[name] = (restype, argtypes)
    return protos


_MEMBER_CTYPES = {
    "int": ctypes.c_int, "int32_t": ctypes.c_int32, "long": ctypes.c_long, "int64_t": ctypes.c_int64, "float": ctypes.c_float,
    "double": ctypes.c_double, "uint16_t": ctypes.c_uint16, "uint8_t": ctypes.c_uint8,
}


def _strip_comments(path):
    src = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return re.sub(r"//[^\n]*", " ", src)


def _struct_class(path, name, body, structs):
    """the ctypes class of one struct body; ``structs``: the classes a member may name"""
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        head = re.match(r"(?:const\s+)?(\w+)\b(.*)", decl, flags=re.S)
        tagged = head and head.group(1) == "struct" and re.match(r"\s*(\w+)\b(.*)", head.group(2), flags=re.S)
        if tagged and issubclass(structs.get(tagged.group(1), int), ctypes.Structure):   # `struct Tag *p`, Tag a struct read before
            head = tagged
        base = head and (structs.get(head.group(1)) or _MEMBER_CTYPES.get(head.group(1)))
        members = [re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?\s*", d) for d in head.group(2).split(",")] if base else [None]
        if not all(members):
            raise ValueError(f"{path}: struct {name}: cannot read the member declaration {decl!r}")
        for star, member, count in (dm.groups() for dm in members):
            t = base if not star else ctypes.POINTER(base) if issubclass(base, ctypes.Structure) else ctypes.c_void_p
            fields.append((member, t * int(count) if count else t))
    return type(name, (ctypes.Structure,), {"_fields_": fields})


def parse_structs(path: str = HEADER):
    """-> {name: ctypes.Structure subclass} for every ``typedef struct ... { ... } Name;`` of the header, in declaration order.  A
    pointer member is c_void_p, a pointer to an earlier struct POINTER(that class), a struct by value that class, ``[N]`` an array.
    A declaration that is none of these raises: a member left out would shift every member behind it."""
    structs = {}
    for m in re.finditer(r"typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;", _strip_comments(path), flags=re.S):
        structs[m.group(2)] = _struct_class(path, m.group(2), m.group(1), structs)
    return structs


def parse_tagged_structs(path: str = HEADER, known=None):
    """-> {tag: ctypes.Structure subclass} for every ``struct Tag { ... };`` of the header that has no typedef name (C callers write
    ``struct Tag``), under the member rules of parse_structs; a member may name a typedef'd struct, or as ``struct Tag`` a tagged one
    read before it.  ``known``: the structs declared in front of ``path`` (a file that the header includes); default: the typedef'd
    structs of ``path`` itself."""
    known = dict(parse_structs(path) if known is None else known)
    out = {}
    for m in re.finditer(r"^struct\s+(\w+)\s*\{(.*?)\}\s*;", _strip_comments(path), flags=re.S | re.M):
        out[m.group(1)] = known[m.group(1)] = _struct_class(path, m.group(1), m.group(2), known)
    return out


def header_abi_version(path: str = HEADER) -> int:
    """VLLM_ABI_VERSION of include/vllm_hip.h (the structs below are parsed from THIS header)."""
    m = re.search(r"^#define\s+VLLM_ABI_VERSION\s+(\d+)", open(path).read(), flags=re.M)
    if not m:
        raise RuntimeError("include/vllm_hip.h: VLLM_ABI_VERSION not found")
    return int(m.group(1))


def lib():
    """Load (once) and return the shared library.  Fails loudly when it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    path = lib_path()
    if not os.path.exists(path):
        raise RuntimeError(
            f"{path} is missing: the HIP extension has not been built. Run `python -c \"import __graft_entry__ as g; "
            "g.build()\"` (or `make -C visionllm_amd/csrc`). There is no CPU fallback.")
    # Load torch FIRST: the extension must bind to the HIP runtime (libamdhip64) that PyTorch-ROCm ships and has
    # initialised.  Loading ours first pulls in /opt/rocm's copy and the two runtimes then disagree about devices
    # ("no ROCm-capable device is detected" at the first launch).
    import torch  # noqa: F401
    L = ctypes.CDLL(path)
    protos = parse_header()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)  # AttributeError if a declared symbol is not exported
        fn.restype = restype
        fn.argtypes = argtypes
    want = header_abi_version()
    if L.vllm_abi_version() != want:
        raise RuntimeError(f"libvllm_hip.so ABI version {L.vllm_abi_version()} != header's VLLM_ABI_VERSION {want}: rebuild "
                           "(make -C visionllm_amd/csrc)")
    _check_struct_layouts(L, protos)
    _lib = L
    return L


def set_option(name: str, value: int) -> int:
    """Process-wide tuning / test knob (see include/vllm_hip.h: vllm_set_option)."""
    return lib().vllm_set_option(name.encode(), int(value))


def check(rc: int, what: str = ""):
    if rc != 0:
        msg = lib().vllm_last_error().decode("utf-8", "replace")
        raise RuntimeError(f"{what or 'libvllm_hip'} failed ({rc}): {msg}")


def aligned(t, align=16):
    """``t`` as a contiguous tensor whose data pointer is a multiple of ``align`` bytes.  A tensor that already is one is returned
    as it is (no copy, so aligned calls launch what they always did); a view at another storage offset is copied into a fresh
    allocation (the caching allocator's blocks start 512-byte aligned).  For entry points that require the alignment."""
    t = t.contiguous()
    if t.data_ptr() % align:
        t = t.clone()
    return t


def ptr(t):
    """Device pointer of a torch tensor (0 for None / empty)."""
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def current_stream(device=None):
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ---- the descriptor structs of include/vllm_hip.h as ctypes classes: _lib.VllmVitDesc, ... (generated, never written by hand) ----
STRUCTS = parse_structs()
globals().update(STRUCTS)
TAGGED_STRUCTS = parse_tagged_structs()          # struct VllmFusionLayerDesc
globals().update(TAGGED_STRUCTS)
GDINO_ENCODER_STRUCTS = parse_tagged_structs(GDINO_ENCODER_HEADER, {**STRUCTS, **TAGGED_STRUCTS})   # struct VllmTextEnhancerDesc, struct VllmGdinoEncoderDesc
globals().update(GDINO_ENCODER_STRUCTS)
GDINO_INPUTS_STRUCTS = parse_tagged_structs(GDINO_INPUTS_HEADER, {**STRUCTS, **TAGGED_STRUCTS, **GDINO_ENCODER_STRUCTS})   # struct VllmGdinoInputsDesc
globals().update(GDINO_INPUTS_STRUCTS)


def pointer_fields(struct):
    """Names of ``struct``'s plain pointer members (no arrays, no pointers to structs), in the header's order: the order in which a
    caller walks the weights, saved tensors or gradients that the struct carries."""
    return tuple(n for n, t in struct._fields_ if t is ctypes.c_void_p)


REGION_PARAMS = pointer_fields(STRUCTS["VllmRegionEncoderGrads"])   # the stem's parameters; VllmRegionEncoder has them in this order too


def _check_struct_layouts(L, protos):
    """Every struct against the library's own sizeof: ``VllmFooBar`` against ``vllm_foo_bar_sizeof()``.  One without such an export
    has to lie by value inside one that has it."""
    checked = []
    for name, cls in {**STRUCTS, **TAGGED_STRUCTS, **GDINO_ENCODER_STRUCTS, **GDINO_INPUTS_STRUCTS}.items():
        fn = "vllm_" + re.sub(r"(?<!^)(?=[A-Z])", "_", name[len("Vllm"):]).lower() + "_sizeof"
        if fn not in protos:
            if name not in STRUCTS:
                raise RuntimeError(f"include/vllm_hip.h: no {fn}() for struct {name}")
            continue
        if ctypes.sizeof(cls) != getattr(L, fn)():
            raise RuntimeError(f"{name}: {ctypes.sizeof(cls)} bytes as parsed from include/vllm_hip.h, {getattr(L, fn)()} in libvllm_hip.so: "
                               "rebuild (make -C visionllm_amd/csrc)")
        checked.append(cls)
    inside = {t._type_ if issubclass(t, ctypes.Array) else t for c in checked for _, t in c._fields_}
    loose =[n for n, cls in STRUCTS.items() if cls not in checked and cls not in inside]
    if loose:
        raise RuntimeError(f"include/vllm_hip.h: no vllm_*_sizeof() covers {', '.join(loose)}")


def check_struct_layouts():
    """The layouts are checked once, when the library is loaded: this loads it."""
    lib()


EPI_BIAS, EPI_GELU, EPI_QUICK_GELU, EPI_RESIDUAL, EPI_EMBED, EPI_F32 = 0, 1, 2, 3, 4, 5
ARCH_INTERNVIT, ARCH_CLIP = 0, 1
BRIDGE_LINEAR, BRIDGE_MLP_GELU, BRIDGE_INTERNVL_MLP = 0, 1, 2

_workspaces = {}


def workspace(device, nbytes, slot=0):
    """Grow-only scratch buffer per (device, caller's current stream, ``slot``) (torch owns the memory; the library never
    allocates).  Keying by stream keeps work enqueued on different streams off each other's scratch: a buffer is only ever
    used by work on the stream it was allocated for, so when it grows the old one goes back to the caching allocator on that
    same stream, behind every kernel that may still read it.  ``slot`` names further independent buffers of one stream (the
    encoder's chunks, which it enqueues on side streams ordered behind the caller's).  Repeated calls on one stream with no
    growth allocate nothing."""
    import torch
    key = (str(device), torch.cuda.current_stream(device).cuda_stream, slot)
    buf = _workspaces.get(key)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(int(nbytes) + 256, dtype=torch.uint8, device=device)
        _workspaces[key] = buf
    return buf


def sized_workspace(device, nbytes, what, slot=0):
    """``workspace()`` for the answer ``nbytes`` of the size query named ``what`` -> (buffer, byte count to pass to C).  A negative
    answer is the query refusing its arguments: raised with the library's error text."""
    check(0 if nbytes >= 0 else -1, what)
    return workspace(device, nbytes, slot), nbytes
