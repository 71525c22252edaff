"""Which kernel a 3x3 convolution runs on -- the one statement of the rule, for inference (pcdet/models/convnet.py::PackedConv.run) and for
the training step (train_layers.fused_f4_choice at pack time, train_layers.launch_conv3x3 at the launch).  Plain ints in, a name out: no
tensors, nothing that needs a GPU.

  conv_algo()             the PCP_CONV_ALGO switch (the only reader of the variable)
  forms_for()             pack time: which weight forms a layer gets
  choose_conv3x3()        launch time: one of KERNELS for a layer on a map
  choose_fused_f4()       the fused F(4x4) part of that rule, which the training step shares
  choose_train_conv3x3()  launch time in the training step: the fused kernel was named at pack time, the rest is decided per launch
"""
import os
from collections import namedtuple

KERNELS = ('direct', 'winograd', 'winograd4', 'winograd4f', 'winograd4h', 'winograd4c', 'bf16x3', 'mp')

# fused Winograd F(2x2,3x3) needs enough workgroups to fill the 256 CUs; below that the direct kernel's smaller tiles win
# (measured on MI355X, tools/bench_conv.py: >= 256 workgroups -> x1.35 .. x2.0 over the direct kernel)
WINOGRAD_MIN_WORKGROUPS = 256
B3_MIN_WORKGROUPS = 256        # the bf16 / bf16x3 conv kernels are used where a launch fills the chip (tests lower it)
# F(4x4,3x3) through memory (three launches, csrc/wino4.hip) wins on the wide layers once its batched GEMM fills the chip twice over
# (tools/bench_conv.py on MI355X, 4 frames: 768->768 @128 x1.50, 384->384 @128 x1.26, 128->384 @128 x1.20, 256->256 @64 x1.16 over the fused
# F(2x2) kernel; narrower outputs or fewer tiles lose)
WINOGRAD4_MIN_COUT = 256
WINOGRAD4_MIN_WORKGROUPS = 512
# the through-memory GEMM pays two extra passes over V and M: measured a win only from 256 input channels and a full 128-wide N tile
# (128 -> 128 @64^2 B = 4: 46 vs 32 us fused F(2x2); 384 -> 64 @128^2: 225 vs 145 us; profiles/r02_bench_conv_b*.txt)
WINOGRAD4_MIN_RUN_CIN = 256
WINOGRAD4_MIN_RUN_COUT = 128
CONV_ALGO = os.environ.get('PCP_CONV_ALGO', 'auto')          # auto | direct | winograd (F(2x2) only) | winograd4 | winograd4f | winograd4h | winograd4c | bf16x3 (opt-in: split-bf16 products) | bf16

# fused F(4x4,3x3) (csrc/wino4f.hip: one workgroup per CU = 16 x 32 pixels x 64 channels): measured against the fused F(2x2) kernel on MI355X
# (tools/bench_conv.py, 4 / 20 frames): 64->64 @256 x1.21 / x1.12, 128->128 @128 x1.34 / x1.36, 384->64 @128 - / x1.41, 384->128 @128 x1.41 /
# x1.46, 128->384 x1.37 / x1.47; it loses when its grid does not fill the chip (128->128 @64 at 4 frames: 64 workgroups) or covers it unevenly
# (320 workgroups on 256 CUs), and the through-memory F(4x4) path keeps the very wide layers (768 -> 768: x0.84)
WINOGRAD4F_MIN_WORKGROUPS = 256
WINOGRAD4F_MAX_CIN = 448
WINOGRAD4H = os.environ.get('PCP_WINO4H', 'auto')          # auto | 0 (never dispatch k_wino4h)
WINOGRAD4H_MAX_CIN = 128
WINOGRAD4H_DEFAULT_MIN_WORKGROUPS = 256
WINOGRAD4H_MIN_WORKGROUPS = int(os.environ.get('PCP_WINO4H_MIN_WGS', WINOGRAD4H_DEFAULT_MIN_WORKGROUPS))
WINOGRAD4F_MAX_INPUT_BYTES = 0x7fffffff                    # buffer-descriptor addressing (tests lower it to exercise the fallback)

_ENV_DATA = getattr(os.environ, '_data', None)           # CPython's backing dict of os.environ (bytes keys on POSIX)
_ENV_KEY = os.environ.encodekey('PCP_CONV_ALGO') if hasattr(os.environ, 'encodekey') else None


def conv_algo():
    """'bf16' (plain bf16 products) is the mixed-precision TRAINING mode (bench.py refuses it without --train): like autocast it also
    covers the frozen teachers' forward passes inside a training iteration; in PackedConv.run it selects the same launches as 'bf16x3'
    with single products.
    Read from the environment at every call (tests and bench.py --optin switch it between forwards) -- through the backing dict:
    os.environ.get() encodes the key and decodes the value every time, ~450 calls and half a millisecond of host time per DiscoNet step."""
    if _ENV_DATA is not None and _ENV_KEY is not None:
        v = _ENV_DATA.get(_ENV_KEY)
        if v is None:
            return CONV_ALGO
        return os.environ.decodevalue(v) if isinstance(v, bytes) else v
    return os.environ.get('PCP_CONV_ALGO', CONV_ALGO)


# ---- workgroups per launch, per 64 (F(4x4) through memory: 128) output channels -----------------------------------------------------------
def _cdiv(a, b):
    return (a + b - 1) // b


def winograd_items(B, H, W):
    """fused F(2x2): the 32-tile instantiation (8 rows x 16 columns of pixels), the finest the library uses"""
    return B * _cdiv(H, 8) * _cdiv(W, 16)


def winograd4_items(B, H, W):
    """through-memory F(4x4): 36 GEMMs over 128-row tiles of 4 x 4-pixel patches"""
    return 36 * _cdiv(B * _cdiv(H, 4) * _cdiv(W, 4), 128)


def winograd4f_items(B, H, W):
    """k_wino4f: 16 x 32 pixels"""
    return B * _cdiv(H, 16) * _cdiv(W, 32)


def winograd4h_items(B, H, W):
    """k_wino4h / k_wino4c: 16 x 16 pixels"""
    return B * _cdiv(H, 16) * _cdiv(W, 16)


def bf16x3_items(B, H, W, stride):
    """16 x 16 output pixels at stride 1, 8 x 16 at stride 2"""
    return B * _cdiv((H - 1) // stride + 1, 16 if stride == 1 else 8) * _cdiv((W - 1) // stride + 1, 16)


# ---- pack time ----------------------------------------------------------------------------------------------------------------------------
_NO_F4_THROUGH_MEMORY = ('direct', 'winograd', 'bf16x3', 'bf16')
_NO_F4_FUSED = ('direct', 'winograd', 'winograd4', 'bf16x3', 'bf16')
_FORCED_F4_FUSED = ('winograd4f', 'winograd4h', 'winograd4c')


def forms_for(cin, cout, stride, algo):
    """the packed weight forms (beside the direct kernel's) a 3x3 layer gets under `algo`: a subset of wino, b3, mp, w4, w4f.  k_wino4h's and
    k_wino4c's forms are repacked from w4f at their first launch; 'mp' (the bf16 loop) also needs the weights on the GPU"""
    from . import pack
    forms = set()
    if stride == 1 and cin % pack.WINO_CK == 0 and cout >= 48:
        forms.add('wino')
    if algo == 'bf16x3' and cin % pack.CK == 0 and cout >= 48:
        forms.add('b3')
    if algo == 'bf16' and cin % 16 == 0 and cout % 8 == 0:
        forms.add('mp')
    if (stride == 1 and cin % pack.WINO4_CK == 0 and cin >= 128 and cout % 4 == 0 and cout >= WINOGRAD4_MIN_COUT
            and algo not in _NO_F4_THROUGH_MEMORY):
        forms.add('w4')
    # layers auto dispatch never sends to the fused kernel (cin above its cap with the through-memory form available) do not get the
    # 4x-sized fused weight form packed at all; PCP_CONV_ALGO=winograd4f packs it for every eligible layer
    if (fused_f4_shape(cin, cout, stride, algo)
            and not (algo not in _FORCED_F4_FUSED and cin > WINOGRAD4F_MAX_CIN and 'w4' in forms)):
        forms.add('w4f')
    return forms


def fused_f4_shape(cin, cout, stride, algo):
    """a layer the fused F(4x4) kernels take, under a switch that does not rule them out"""
    return stride == 1 and cin % 8 == 0 and cout % 4 == 0 and cout >= 48 and algo not in _NO_F4_FUSED


# ---- launch time --------------------------------------------------------------------------------------------------------------------------
# cout_pad of each packed form a layer has, None where it has none
Forms = namedtuple('Forms', 'wino b3 w4 w4f mp', defaults=(None,) * 5)


def choose_fused_f4(algo, cin, w4f_pad, has_w4, B, H, W, ld_in=4, in_ch_off=0, out_ld=None, out_ch_off=0, *, kernel_limits=True,
                    knows_4c=True, wino4h_overrides=True, cap_needs_w4=True, half_before_cap=False):
    """None | 'winograd4f' | 'winograd4h' | 'winograd4c' for a stride-1 layer whose fused form exists (w4f_pad: its cout_pad).
    Which of the fused kernels: the half-size items (two four-wave workgroups per CU, 16 x 16 pixels: one workgroup's prologue / epilogue
    under the other's MFMAs) or k_wino4f (one eight-wave workgroup, 16 x 32-pixel items: half the weight traffic per product).
    Interleaved A/B on MI355X (tools/bench_w4h.py, profiles/r03_wino4h_ab.txt): 4h wins up to 128 input channels wherever its
    grid covers the chip (>= 256 workgroups), by 3-4 % on full grids and 20-40 % on the grids 4f fills unevenly; 4f keeps cin >= 256.
    The half-size kernel is k_wino4c (round 4: waves split over the output channels, output transform in registers; the bits of
    k_wino4h, 2 - 6 % faster on every shape of the step, profiles/r04_wino4c_ab.txt) unless k_wino4h is asked for by name.

    The keyword arguments are the places where the training step's copy of this rule had drifted from inference; inference leaves them all
    at their defaults, train_layers.fused_f4_choice sets all five.  Each is inherited, not measured:"""
    # kernel_limits=False     inherited: training checks the kernels' alignment / 2 GiB limits at the launch, not in the choice
    # knows_4c=False          inherited: training has no k_wino4c -- 'winograd4c' is an unknown value there, half-size items mean k_wino4h
    # wino4h_overrides=False  inherited: training ignores PCP_WINO4H and PCP_WINO4H_MIN_WGS
    # cap_needs_w4=False      inherited: training applies the cin <= 448 cap whether or not a through-memory form exists
    # half_before_cap=True    inherited: training tests the half-size kernel before the cap, inference after
    if w4f_pad is None or algo in _NO_F4_FUSED:
        return None
    if kernel_limits:
        if out_ld is not None and (out_ld % 4 != 0 or out_ch_off % 4 != 0):
            return None                                    # 16-byte output stores
        # the kernel's own limits (csrc/wino4f.hip f4_geom): 16-byte input loads through a buffer descriptor with 32-bit byte offsets.
        # Outside them the launch returns PCP_ERR_UNSUPPORTED / PCP_ERR_ARG, so the dispatch falls through to the other kernels instead
        if ld_in % 4 != 0 or in_ch_off % 4 != 0 or B * H * W * ld_in * 4 > WINOGRAD4F_MAX_INPUT_BYTES:
            return None
    if algo in ('winograd4f', 'winograd4h') or (algo == 'winograd4c' and knows_4c):
        return algo
    nb = w4f_pad // 64
    wgs = winograd4f_items(B, H, W) * nb
    capped = cin > WINOGRAD4F_MAX_CIN and (has_w4 or not cap_needs_w4)
    if capped and not half_before_cap:
        return None
    # the half-size items also cover grids k_wino4f fills unevenly; wider layers only where the eight-wave kernel's 16 x 32-pixel items leave
    # CUs idle (CenterHead's 384 -> 64 conv at 4 frames: 128 items; k_wino4h 95 us against 145 us on the fused F(2x2) kernel that used to
    # take it, tools/bench_conv.py)
    if (not (wino4h_overrides and WINOGRAD4H == '0')
            and winograd4h_items(B, H, W) * nb >= (WINOGRAD4H_MIN_WORKGROUPS if wino4h_overrides else WINOGRAD4H_DEFAULT_MIN_WORKGROUPS)
            and (cin <= WINOGRAD4H_MAX_CIN or wgs < WINOGRAD4F_MIN_WORKGROUPS)):
        return 'winograd4c' if knows_4c else 'winograd4h'
    if capped:
        return None
    if H * W <= 64 * 64 and cin <= 128:
        return None                                        # 8 spatial tiles per frame, 16 K slices: F(2x2) wins (profiles/r02_bench_conv_b*.txt)
    return 'winograd4f' if wgs >= WINOGRAD4F_MIN_WORKGROUPS and (wgs % 256 == 0 or wgs >= 512) else None


def choose_conv3x3(algo, cin, cout, stride, forms, B, H, W, ld_in, in_ch_off=0, out_ld=None, out_ch_off=0, in_fp32=True):
    """one of KERNELS for a 3x3 layer cin -> cout (forms: Forms) on a (B, H, W, ld_in) map read from channel in_ch_off and written at channel
    out_ch_off of a buffer of out_ld channels (None: the launch allocates its output).  Decided per call: it depends on the launch size."""
    if forms.mp is not None and algo == 'bf16':
        return 'mp'                                        # the bf16 loop takes any input: it casts what it needs
    if not in_fp32:
        ld_in, in_ch_off = cin, 0                          # the fp32 kernels get a contiguous float copy of the channel window
    # opt-in only (PCP_CONV_ALGO=bf16x3), and only where the launch fills the chip (>= 256 workgroups of 16x16 px x 64 ch)
    if forms.b3 is not None and algo in ('bf16x3', 'bf16') and bf16x3_items(B, H, W, stride) * (forms.b3 // 64) >= B3_MIN_WORKGROUPS:
        return 'bf16x3'
    f4 = choose_fused_f4(algo, cin, forms.w4f, forms.w4 is not None, B, H, W, ld_in, in_ch_off, out_ld, out_ch_off)
    if f4 is not None:
        return f4
    if forms.w4 is not None and algo not in _NO_F4_THROUGH_MEMORY:
        if algo == 'winograd4' or (cin >= WINOGRAD4_MIN_RUN_CIN and cout >= WINOGRAD4_MIN_RUN_COUT
                                   and winograd4_items(B, H, W) * (forms.w4 // 128) >= WINOGRAD4_MIN_WORKGROUPS):
            return 'winograd4'
    if forms.wino is not None and algo != 'direct':
        if algo == 'winograd' or winograd_items(B, H, W) * (forms.wino // 64) >= WINOGRAD_MIN_WORKGROUPS:
            return 'winograd'
    return 'direct'


def choose_train_conv3x3(algo, stride, forms, fused, B, H, W, ld_in, in_ch_off, out_ld, out_ch_off):
    """'bf16x3' | 'winograd4f' | 'winograd4h' | 'winograd' | 'direct' for a 3x3 conv of the training step (forward, or the stride-1 data-gradient
    conv) on a (B, H, W, ld_in) fp32 map.  forms: Forms with the cout_pad of the b3 and wino forms the layer has.  fused: None | 'winograd4f' |
    'winograd4h', the kernel train_layers.fused_f4_choice named when the fused form was packed (from the LAYER's input map); only that
    kernel's own limits -- 16-byte windows, 32-bit buffer offsets -- are left to test here."""
    if forms.b3 is not None and algo in ('bf16x3', 'bf16') and bf16x3_items(B, H, W, stride) * (forms.b3 // 64) >= B3_MIN_WORKGROUPS:
        return 'bf16x3'
    if (fused is not None and stride == 1 and ld_in % 4 == 0 and in_ch_off % 4 == 0 and out_ld % 4 == 0 and out_ch_off % 4 == 0
            and B * H * W * ld_in * 4 <= WINOGRAD4F_MAX_INPUT_BYTES):
        return fused
    if forms.wino is not None and stride == 1 and algo != 'direct':
        if algo == 'winograd' or winograd_items(B, H, W) * (forms.wino // 64) >= WINOGRAD_MIN_WORKGROUPS:
            return 'winograd'
    return 'direct'
