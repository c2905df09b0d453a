"""The grid of layers that tests/test_conv_plan_host.py holds nf_conv_plan to, and how one of them is asked.

Shared by the test and by tests/golden/make_golden_conv_plan.py, which recorded tests/golden/conv_plan.json.  The full
product of the axes below is some 200,000 layers; the grid is the union of five cuts through it, each full in the axes
that interact (a few thousand layers in all):
  A  every lattice x every kernel: all (cin, cout) for kernel 3, the PAIRS for the others; plain fp32 output, batch 1
  B  every lattice x kernels 3 and (3,3,3,5) x PAIRS x compact 0, 1, 2 x (fp32 at batch 1 and 65535, fp64 at batch 1)
  C  fused 1, 3, 7 x every lattice x FUSED_PAIRS (kernel 3; kernel 5 for 8 -> 46) x (fp32 x the three option sets x batch
     1 and 65535, fp64 at batch 1)
  D  the option sets other than the default x every lattice x kernel 3 x PAIRS x compact 0, 1
  E  every lattice x kernel 5 x PAIRS in fp64 (the boxes that outgrow the LDS)
A kernel is cut to the lattice's number of axes from the right: (3,3,3,5) is (3,5) on a 2-d lattice."""
import itertools


from normflow__amd import _hip

LATTICES = [(16,), (8, 8), (16, 16), (4, 6, 16), (16, 16, 16), (5, 7, 9), (8, 8, 8, 16), (4, 4, 4, 32), (2, 2, 2, 64),
            (2, 2, 2, 48), (6, 6, 6, 48), (32, 32, 32, 32), (48, 48, 48, 48)]
KERNELS = [(1, 1, 1, 1), (3, 3, 3, 3), (5, 5, 5, 5), (3, 3, 3, 5)]
K3 = KERNELS[1]
CIN = [1, 2, 6, 8, 12, 16]
COUT = [1, 8, 20, 46, 52]
PAIRS = [(1, 8), (2, 20), (8, 8), (8, 46), (12, 52), (16, 20)]
FUSED_PAIRS = [(8, 46), (8, 22), (16, 46), (6, 10), (8, 20)]
COMPACT = [0, 1, 2]
FUSED = [0, 1, 3, 7]
DTYPES = [_hip.NF_F32, _hip.NF_F64]
OPTIONS = [dict(split16=True, pipe=True), dict(split16=False, pipe=True), dict(split16=False, pipe=False)]
BATCHES = [1, 65535]

# a case: (lattice, kernel, cin, cout, compact, fused, dtype code, index into OPTIONS, batch)
# a plan: (return code, index into the file's list of message starts or -1, then the fields of _hip.ConvPlan in order,
# box and nbox as four entries each); a refused layer has zeros for the fields
MESSAGE_START = 32      # characters of nf_last_error_string kept for a refusal


def cases():
    seen, out = set(), []

    def add(*case):
        if case not in seen:
            seen.add(case)
            out.append(case)

    f32, f64 = DTYPES
    for lat in LATTICES:
        for k in KERNELS:
            for cin, cout in (itertools.product(CIN, COUT) if k == K3 else PAIRS):
                add(lat, k, cin, cout, 0, 0, f32, 0, 1)
        for k, (cin, cout), compact in itertools.product((K3, KERNELS[3]), PAIRS, COMPACT):
            for dtype, B in ((f32, 1), (f32, 65535), (f64, 1)):
                add(lat, k, cin, cout, compact, 0, dtype, 0, B)
        for fused, (k, (cin, cout)) in itertools.product(FUSED[1:], [(K3, p) for p in FUSED_PAIRS] + [(KERNELS[2], (8, 46))]):
            for opt, B in itertools.product(range(len(OPTIONS)), BATCHES):
                add(lat, k, cin, cout, 1, fused, f32, opt, B)
            add(lat, k, cin, cout, 1, fused, f64, 0, 1)
        for opt, (cin, cout), compact in itertools.product((1, 2), PAIRS, (0, 1)):
            add(lat, K3, cin, cout, compact, 0, f32, opt, 1)
        for cin, cout in PAIRS:
            add(lat, KERNELS[2], cin, cout, 0, 0, f64, 0, 1)
    return out


def plan_of(case, messages):
    """The plan row of `case`; the start of a refusal's message is looked up in, or appended to, `messages`."""
    lat, k, cin, cout, compact, fused, dtype, opt, B = case
    lat4, k4 = _hip._lat4(list(lat), list(k[4 - len(lat):]))
    out = _hip.ConvPlan()
    lib = _hip.load()
    with _hip.options(**OPTIONS[opt]):
        rc = lib.nf_conv_plan(lat4, k4, cin, cout, compact, fused, dtype, B, _hip.C.byref(out))
    if rc:
        msg = lib.nf_last_error_string().decode()[:MESSAGE_START]
        if msg not in messages:
            messages.append(msg)
        return [rc, messages.index(msg)] + [0] * 18
    row = [0, -1]
    for name, _ in _hip.ConvPlan._fields_:
        v = getattr(out, name)
        row += list(v) if name in ("box", "nbox") else [v]
    return row
