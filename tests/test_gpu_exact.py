"""Exact-lattice tests of the GEMM family (MI355X): every element, no tolerance.

The operands come from the dyadic lattices of tests/exact_lattice.py, on which every partial sum of a launch, in any order, is exactly representable in
fp32 (asserted per case as ``budget < 2^24`` before anything is launched: a precondition on the inputs, not a tolerance).  The result then does not depend
on the accumulation order, the tile shape, the MFMA variant or the split-K count, so each output element has ONE correct bit pattern, which an fp64
evaluation of the operation's definition gives: out32 is the exact value, out16 its round-to-nearest-even fp16, an emitted plane set is mxfp4.py applied to
the exact value after the consumer's slope, byte for byte.  Unlike the kernel-against-kernel comparisons of test_gpu_ops.py the reference shares no code
with the kernels, and unlike the whole-tensor norms one wrong element fails.

Every kernel is reached through ev_op_conv_gemm (and ev_op_conv_gemm_group3) at the smallest shape its launcher rule allows (launch_dt, launch_phased,
launch_split, mx_launch_kind in ev_gemm.hip; the case's ``kernel`` field names the target).  Long-M cases take their reference from torch fp64 on the
device (a sum over taps of shifted x @ w_t.T: exact on the lattice, none of this project's kernels involved) after a few hundred of its rows, both ends and a
tile edge included, were checked against the CPU evaluation.  The negative controls evaluate a deliberately different problem (dil + 1, centre off by one,
two taps swapped, one scale byte of an input plane set changed) and assert that the comparison reports mismatches: the lattices are not so sparse or
symmetric that errors cancel.  exact_report.json, written next to parity_report.json, records kernel, shape, lattice, budget, elements compared and mismatches per case.

The fused ResBlock pair kernels follow at the end of the file, through the harness classes of test_gpu_pair_long.py.

GELU, tanh and non-dyadic scales (the engine's 1/3) stay with the tolerance tests.  Not reachable through the entry points without tuning environment
variables: conv_gemm_split_kernel at BN = 32 (launch_split sends every N % 64 != 0 call to conv_gemm_x3_kernel)."""
import ctypes as C

import numpy as np
import pytest

import exact_lattice as EL
from exact_lattice import PAD, Case

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

from test_gpu_ops import _PlaneSet, lib      # noqa: E402, F401  (lib: the module-scoped library fixture)
from test_gpu_parity import _report as write_report      # noqa: E402

REPORT = {}
SENT = 7.0
LONG_FLOP = 4e9          # above this a case takes its reference from torch fp64 on the device


def _c(name, kernel, dtype, M, K, N, taps, dil=1, **kw):
    return Case(name, kernel, dtype, M, K, N, taps, dil, **kw)


def _edge_run(shift, row=256):
    """an invalid run of three row groups that starts in the tile before ``row`` and crosses it"""
    return ((row >> shift) - 1, 3)


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# dtype 0 (fp16), lattice L0
F16_TILE_CASES = [
    _c("f16_256x32_c32_k11_d5", "conv_gemm_kernel<256,32>", 0, 512, 32, 32, 11, 5, mask=2, mask_runs=(_edge_run(2),)),
    _c("f16_256x32_n96_k3", "conv_gemm_kernel<256,32>", 0, 256, 64, 96, 3),
    _c("f16_256x64_c64_k7_d3", "conv_gemm_kernel<256,64>", 0, 512, 64, 64, 7, 3, mask=3, mask_runs=(_edge_run(3),)),
    _c("f16_latency_c128_k3", "conv_gemm_kernel<256,32> (latency configuration)", 0, 512, 128, 128, 3, mask=4, mask_runs=(_edge_run(4),)),
    _c("f16_128x128_n1536", "conv_gemm_kernel<128,128>", 0, 1536, 128, 1536, 3),
    _c("f16_256x128_n1536", "conv_gemm_kernel<256,128>", 0, 5632, 128, 1536, 3),          # 264 tiles; both outputs: no phased variant
]

_MRF = ("bias", "res16", "scale", "add16", "post", "before_post")
# every fp16 epilogue instantiation of launch_cfg (fp16_epi_variant), the generic one via seq_bias and via acc32
F16_EPI_CASES = [
    _c("epi_0", "EPI 0", 0, 512, 64, 128, 3, epi=("bias", "pro", "lrelu")),
    _c("epi_o16", "EPI_O16", 0, 512, 64, 64, 3, epi=("bias", "pro", "lrelu"), outs="16", slope=0.125),
    _c("epi_o32", "EPI_O32", 0, 512, 64, 128, 3, outs="32"),
    _c("epi_rare", "EPI_RARE_ACT", 0, 512, 64, 64, 3, epi=("bias", "relu")),
    _c("epi_rare_o16", "EPI_RARE_ACT | EPI_O16", 0, 512, 64, 128, 3, epi=("bias", "relu"), outs="16"),
    _c("epi_res16", "EPI_RES16", 0, 512, 64, 64, 3, epi=("bias", "res16")),
    _c("epi_res16_o16", "EPI_RES16 | EPI_O16", 0, 512, 64, 128, 3, epi=("bias", "res16"), outs="16", mask=3, mask_runs=(_edge_run(3),)),
    _c("epi_res16_o32", "EPI_RES16 | EPI_O32", 0, 512, 64, 64, 3, epi=("bias", "res16", "scale"), outs="32", scale=0.25),
    _c("epi_res16_add16", "EPI_RES16 | EPI_ADD16", 0, 512, 64, 128, 3, epi=_MRF, mask=3),
    _c("epi_res16_add16_o16", "EPI_RES16 | EPI_ADD16 | EPI_O16", 0, 512, 64, 64, 3, epi=_MRF, outs="16", slope=0.125),
    _c("epi_res32", "EPI_RES32", 0, 512, 64, 128, 3, epi=("bias", "res32")),
    _c("epi_res32_o32", "EPI_RES32 | EPI_O32", 0, 512, 64, 64, 3, epi=("bias", "res32"), outs="32"),
    _c("epi_generic_seq_bias", "EPI_GENERIC (seq_bias)", 0, 512, 64, 128, 3, epi=("bias", "lrelu", "seq_bias", "post")),
    _c("epi_generic_acc32", "EPI_GENERIC (acc32)", 0, 512, 64, 64, 7, 3, epi=("bias", "pro", "res16", "scale", "acc32", "post", "before_post"), scale=0.25,
       mask=3, mask_runs=(_edge_run(3),)),
]

# conv_gemm_phased_kernel: 3 / 7 / 11 taps at BN 128 (>= 256 tiles of 256 x 128: 12 column tiles x 22), 11 taps at BN 64 (>= 512 tiles), its five
# epilogue variants; each launch again with reserved0 bit 2 (the 4-wave kernel on the same problem)
_PH = dict(dtype=0, M=5632, K=128, N=1536)
_PH64 = dict(dtype=0, M=131072, K=64, N=64)
PHASED_CASES = [
    Case("ph_k3_pro", "conv_gemm_phased_kernel<3,128,EPI_O16>", taps=3, epi=("bias", "pro", "lrelu"), outs="16", **_PH),
    Case("ph_k3_res16_masked", "conv_gemm_phased_kernel<3,128,EPI_RES16|EPI_O16>", taps=3, epi=("bias", "res16"), outs="16", mask=2, mask_runs=(_edge_run(2, 1024),), **_PH),
    Case("ph_k3_mrf", "conv_gemm_phased_kernel<3,128,EPI_RES16|EPI_ADD16|EPI_O16>", taps=3, epi=_MRF, outs="16", **_PH),
    Case("ph_k3_relu", "conv_gemm_phased_kernel<3,128,EPI_RARE_ACT|EPI_O16>", taps=3, epi=("bias", "relu"), outs="16", **_PH),
    Case("ph_k3_res32", "conv_gemm_phased_kernel<3,128,EPI_RES32|EPI_O32>", taps=3, epi=("bias", "res32"), outs="32", **_PH),
    Case("ph_k7_d3_res16_masked", "conv_gemm_phased_kernel<7,128,EPI_RES16|EPI_O16>", taps=7, dil=3, epi=("bias", "res16"), outs="16", mask=3, mask_runs=(_edge_run(3, 2048),), **_PH),
    Case("ph_k7_relu", "conv_gemm_phased_kernel<7,128,EPI_RARE_ACT|EPI_O16>", taps=7, epi=("bias", "relu"), outs="16", **_PH),
    Case("ph_k7_d1_pro", "conv_gemm_phased_kernel<7,128,EPI_O16>", taps=7, epi=("bias", "pro", "lrelu"), outs="16", slope=0.125, **_PH),
    Case("ph_k11_d5_mrf", "conv_gemm_phased_kernel<11,128,EPI_RES16|EPI_ADD16|EPI_O16>", taps=11, dil=5, epi=_MRF, outs="16", mask=4, mask_runs=(_edge_run(4, 512),), **_PH),
    Case("ph_k11_d1_pro", "conv_gemm_phased_kernel<11,128,EPI_O16>", taps=11, epi=("bias", "pro", "lrelu"), outs="16", **_PH),
    Case("ph_k11_d6_res16", "conv_gemm_phased_kernel<11,128,EPI_RES16|EPI_O16>", taps=11, dil=6, epi=("bias", "res16"), outs="16", **_PH),
    Case("ph64_k11_d5_pro", "conv_gemm_phased_kernel<11,64,EPI_O16>", taps=11, dil=5, epi=("bias", "pro", "lrelu"), outs="16", **_PH64),
    Case("ph64_k11_d1_res16", "conv_gemm_phased_kernel<11,64,EPI_RES16|EPI_O16>", taps=11, epi=("bias", "res16"), outs="16", mask=3, mask_runs=(_edge_run(3, 65536),), **_PH64),
    Case("ph64_k11_d3_mrf", "conv_gemm_phased_kernel<11,64,EPI_RES16|EPI_ADD16|EPI_O16>", taps=11, dil=3, epi=_MRF, outs="16", **_PH64),
]

# dtype 1 (fp32 MFMA), lattice L0: the four tile configurations; <256,128> needs >= 2048 tiles (64 column tiles x 32)
F32_CASES = [
    _c("f32_256x32_k7", "conv_gemm_kernel<float,256,32>", 1, 256, 32, 32, 7, epi=("bias", "lrelu", "res32", "scale", "acc32", "post", "before_post"), mask=2),
    _c("f32_256x64_k3", "conv_gemm_kernel<float,256,64>", 1, 512, 64, 64, 3, 5, epi=("bias", "relu"), mask=3, mask_runs=(_edge_run(3),)),
    _c("f32_128x128_seq_bias", "conv_gemm_kernel<float,128,128>", 1, 256, 384, 384, 1, epi=("bias", "lrelu", "seq_bias"), outs="32"),
    _c("f32_128x128_k3", "conv_gemm_kernel<float,128,128>", 1, 512, 128, 256, 3, epi=("bias", "pro", "res32")),
    _c("f32_256x128_n8192", "conv_gemm_kernel<float,256,128>", 1, 8192, 32, 8192, 1, outs="32"),
]

# dtype 2 (split precision: three fp16 MFMAs per product), both lattices
_FULL32 = ("bias", "relu", "res32", "scale", "acc32", "post")


def _x3_cases(lat, dens):
    d = dict(dtype=2, lattice=lat, outs="32")
    n = lambda s: "x3_%s_%s" % (lat, s)          # noqa: E731
    return [
        Case(n("split64_o32"), "conv_gemm_split_kernel<128,64,EPI_O32>", M=512, K=128, N=128, taps=3, density=dens[0], **d),
        Case(n("split64_pro_lrelu"), "conv_gemm_split_kernel<128,64,EPI_O32>", M=512, K=64, N=64, taps=7, dil=3, epi=("bias", "pro", "lrelu"), density=dens[1], mask=2,
             mask_runs=(_edge_run(2, 128),), **d),
        Case(n("split64_relu"), "conv_gemm_split_kernel<128,64,EPI_RARE_ACT|EPI_O32>", M=256, K=128, N=128, taps=3, epi=("bias", "relu"), density=dens[0], **d),
        Case(n("split64_res32"), "conv_gemm_split_kernel<128,64,EPI_RES32|EPI_O32>", M=256, K=128, N=128, taps=3, epi=("bias", "res32"), density=dens[0], **d),
        Case(n("split64_res32_acc32"), "conv_gemm_split_kernel<128,64,EPI_RES32|EPI_ACC32|EPI_O32>", M=256, K=128, N=128, taps=3, epi=("bias", "res32", "scale", "acc32"),
             density=dens[0], mask=3, **d),
        Case(n("split64_generic"), "conv_gemm_split_kernel<128,64,EPI_GENERIC>", M=256, K=128, N=128, taps=11, epi=_FULL32 + ("before_post",), density=dens[2], dtype=2, lattice=lat),
        Case(n("bn32_k11_d5"), "conv_gemm_x3_kernel<32>", M=512, K=32, N=32, taps=11, dil=5, epi=("bias", "pro", "lrelu"), density=dens[1], mask=2, mask_runs=(_edge_run(2),), **d),
        Case(n("bn32_n96_res32_acc32"), "conv_gemm_x3_kernel<32,EPI_RES32|EPI_ACC32|EPI_O32>", M=256, K=64, N=96, taps=3, epi=("bias", "res32", "scale", "acc32"), density=dens[1], **d),
        Case(n("bn128_n1536"), "conv_gemm_x3_kernel<128>", M=11008, K=64, N=1536, taps=3, epi=("bias", "res32"), density=dens[1], **d),
        Case(n("bn64_n448_k7_d3"), "conv_gemm_x3_kernel<64>", M=18944, K=64, N=448, taps=7, dil=3, epi=("bias", "pro", "lrelu"), density=dens[1], mask=3,
             mask_runs=(_edge_run(3, 4096),), **d),
        Case(n("bn64_generic"), "conv_gemm_x3_kernel<64,EPI_GENERIC>", M=18944, K=32, N=448, taps=3, epi=_FULL32, density=dens[1], dtype=2, lattice=lat),
    ] + [Case(n("splitk_s%d" % S), "conv_gemm_split_kernel (ksplit %d) + splitk_reduce_kernel" % S, M=256, K=384, N=128, taps=3, epi=_FULL32, density=dens[3], mask=3, ksplit=S,
              dtype=2, lattice=lat, outs="both" if S == 3 else "32") for S in (2, 3, 12)]          # 12 K-chunks: S = 12 is one chunk per range


# L1 densities (probability of a nonzero hi part) per (K x taps) class, lowered until budget() holds: [K 128 x 3, K <= 64, K 128 x 11, K 384 x 3]
X3_CASES = _x3_cases("L0", (1.0, 1.0, 1.0, 1.0)) + _x3_cases("L1", (0.17, 0.16, 0.07, 0.09))

# dtype 3 (MX: one fp16 MFMA + two block-scaled fp4 MFMAs per product), both lattices.  extra: "planes_in" = the input is a plane set built by the host
# quantiser (otherwise fp32 through mx_planes_kernel); "mxo" = the launch emits the plane set of its result; "up<s>" = a transposed conv of stride s with the
# polyphase hint; "r0=<bits>" = reserved0 (kernel selection at C = 64)
def _mx_cases(lat, dens):
    d = dict(dtype=3, lattice=lat, outs="32")
    n = lambda s: "mx_%s_%s" % (lat, s)          # noqa: E731
    cs = []
    for taps, dil, dn in ((3, 1, dens[0]), (7, 3, dens[1]), (11, 5, dens[2])):
        kern = "conv_gemm_mx_kernel<%d>" % taps
        cs.append(Case(n("k%d_f32in" % taps), "mx_planes_kernel + " + kern, M=512, K=128, N=128, taps=taps, dil=dil, epi=("bias", "pro", "lrelu"), density=dn, mask=2,
                       mask_runs=(_edge_run(2),), **d))
        cs.append(Case(n("k%d_planes_in_mxo" % taps), kern + " (EPI_O32|EPI_MXP)", M=512, K=128, N=128, taps=taps, dil=dil, epi=("bias", "lrelu"), density=dn, mask=3,
                       mask_runs=(_edge_run(3),), extra=("planes_in", "mxo"), **d))
    cs += [
        Case(n("k3_c256_res32_acc32"), "conv_gemm_mx_kernel<3> (EPI_RES32|EPI_ACC32|EPI_O32)", M=256, K=256, N=256, taps=3, dil=5, epi=("bias", "res32", "scale", "acc32"),
             density=dens[3], extra=("planes_in",), **d),
        Case(n("k7_res32_mxo"), "conv_gemm_mx_kernel<7> (EPI_RES32|EPI_O32|EPI_MXP)", M=256, K=128, N=256, taps=7, epi=("bias", "res32"), density=dens[1], extra=("mxo",), **d),
        Case(n("k3_all_gap_tile"), "conv_gemm_mx_kernel<3>, an all-gap tile", M=1024, K=128, N=128, taps=3, density=dens[0], mask=6, mask_runs=((4, 4),), extra=("mxo",), **d),
        Case(n("mx1"), "gemm_mx1_kernel<EPI_O32>", M=768, K=384, N=384, taps=1, density=dens[4], mask=6, mask_runs=((4, 4),), **d),
        Case(n("mx1_res32"), "gemm_mx1_kernel<EPI_RES32|EPI_O32>", M=512, K=128, N=256, taps=1, epi=("bias", "res32"), density=dens[5], **d),
        Case(n("up4"), "conv_gemm_mx_up_kernel<EPI_O32|EPI_MXP>", M=512, K=256, N=512, taps=3, epi=("bias", "pro"), density=dens[6], mask=2, extra=("up4", "mxo"), **d),
    ]
    # the residual from a plane set (EPI_RESPL) and the MRF sum as partial plane sets (EPI_ACCPL / EPI_PART): every epilogue variant of mx_epi_variant
    rp = dict(M=512, K=128, N=128, dtype=3, lattice=lat, mask=3, mask_runs=(_edge_run(3),))
    for i, (form, epi, outs_, extra) in enumerate((
            ("RESPL|MXP", ("bias", "respl", "scale"), "none", ("mxo",)),
            ("RESPL|O32", ("bias", "respl", "scale"), "32", ()),
            ("RESPL|O32|MXP", ("bias", "respl", "scale"), "32", ("mxo",)),
            ("RESPL|ACC32|O32", ("bias", "respl", "scale", "acc32"), "32", ()),
            ("RESPL|ACC32|O32|MXP", ("bias", "respl", "scale", "acc32"), "32", ("mxo",)),
            ("RESPL|ACC32|MXP", ("bias", "respl", "scale", "acc32"), "none", ("mxo",)),
            ("RESPL|MXP|PART", ("bias", "respl", "scale"), "none", ("mxo", "partial")),
            ("RESPL|ACCPL|MXP|PART", ("bias", "respl", "scale", "accpl"), "none", ("mxo", "partial", "inplace")),
            ("RESPL|ACCPL|MXP", ("bias", "respl", "scale", "accpl"), "none", ("mxo",)))):
        taps, dil, dn = ((3, 1, dens[0]), (7, 3, dens[1]), (11, 1, dens[2]))[i % 3]
        cs.append(Case(n("respl%d_k%d" % (i, taps)), "conv_gemm_mx_kernel<%d> (%s)" % (taps, form), taps=taps, dil=dil, density=dn, epi=epi, outs=outs_,
                       extra=("planes_in",) + extra, slope=(0.5, 0.125)[i % 2], scale=(0.5, 0.25)[i % 2], **rp))
    for taps, dil, dn, r0, epi, outs_, extra in ((3, 5, dens[7], 0, ("bias", "respl", "scale"), "none", ("mxo",)), (7, 1, dens[8], 8, ("bias", "respl", "scale", "acc32"), "32", ("mxo",)),
                                                 (11, 5, dens[9], 12, ("bias", "respl", "scale"), "32", ()), (7, 3, dens[8], 0, ("bias", "respl", "scale", "acc32"), "32", ("mxo",))):
        kern = {0: "conv_c64_mx2_kernel" if taps == 3 else "conv_gemm_mx64_kernel", 8: "conv_c64_mx2_kernel", 12: "conv_c64_mx_kernel"}[r0]
        cs.append(Case(n("c64_respl_k%d_r%d" % (taps, r0)), "%s<%d>, residual from planes" % (kern, taps), M=768, K=64, N=64, taps=taps, dil=dil, density=dn, epi=epi, outs=outs_,
                       mask=3, mask_runs=(_edge_run(3),), extra=("planes_in", "r0=%d" % r0) + extra, dtype=3, lattice=lat))
    for taps, dil, dn in ((3, 1, dens[7]), (7, 3, dens[8]), (11, 5, dens[9])):
        for r0, kern in ((0, "conv_c64_mx2_kernel" if taps == 3 else "conv_gemm_mx64_kernel"), (8, "conv_c64_mx2_kernel"), (4 | 8, "conv_c64_mx_kernel")):
            if taps == 3 and r0 == 8:
                continue
            cs.append(Case(n("c64_k%d_r%d" % (taps, r0)), "%s<%d>" % (kern, taps), M=768, K=64, N=64, taps=taps, dil=dil, epi=("bias", "lrelu") if r0 != 8 else ("bias", "res32", "scale", "acc32"),
                           density=dn, mask=3, mask_runs=(_edge_run(3),), extra=("planes_in", "mxo", "r0=%d" % r0) if r0 != 8 else ("planes_in", "r0=%d" % r0), **d))
    return cs


_ONES10 = (1.0,) * 10
# [K128 x 3, K128 x 7, K128 x 11, K256 x 3, K384 x 1, K128 x 1, up K256 x 3, C64 x 3, C64 x 7, C64 x 11]
MX_CASES = _mx_cases("L0", _ONES10) + _mx_cases("L1", (0.15, 0.1, 0.08, 0.11, 0.17, 0.28, 0.14, 0.2, 0.14, 0.11))

# the engine's grouped triple (conv1 of the three ResBlock branches of a stage: planes in, planes only out)
# and conv2 inside the ResBlocks: the residual from a plane set, planes only out)
GROUP3_CASES = [tuple(Case("g3_%s_%s_k%d" % (form, lat, taps), "conv_gemm_mx_group3_kernel<%s>" % kern, 3, 768, 128, 128, taps, dil if form == "conv1" else 1, lattice=lat, density=dn, epi=epi,
                           outs="none", mask=3, mask_runs=(_edge_run(3),), extra=("planes_in", "mxo"), seed=5) for taps, dil, dn in ((11, 5, dens[2]), (7, 3, dens[1]), (3, 1, dens[0])))
                for lat, dens in (("L0", (1.0, 1.0, 1.0)), ("L1", (0.15, 0.1, 0.08)))
                for form, kern, epi in (("conv1", "EPI_MXP", ("bias", "lrelu")), ("conv2", "EPI_RESPL|EPI_LEAN|EPI_MXP", ("bias", "respl", "scale")))]

ALL_CASES = F16_TILE_CASES + F16_EPI_CASES + PHASED_CASES + F32_CASES + X3_CASES + MX_CASES + [c for t in GROUP3_CASES for c in t]
NEGATIVE_CASES = [c for c in ALL_CASES if c.name in ("f16_256x64_c64_k7_d3", "epi_generic_acc32", "f32_256x64_k3", "x3_L0_split64_pro_lrelu", "x3_L1_bn32_k11_d5",
                                                     "x3_L1_splitk_s3", "mx_L0_k7_f32in", "mx_L1_k7_f32in", "mx_L1_c64_k7_r0")]
assert len({c.name for c in ALL_CASES}) == len(ALL_CASES) and len(NEGATIVE_CASES) == 9


def _ids(cases):
    return [c.name for c in cases]


def case_inputs(case):
    """make_inputs, plus what the MX forms need: a transposed conv's weight in its 3-tap GEMM layout (structural zeros in one tap per phase)"""
    inp = EL.make_inputs(case)
    up = [e for e in case.extra if e.startswith("up")]
    if up:
        from emotivoice_amd.packer import _convT_to_gemm
        s = int(up[0][2:])
        cout = case.N // s
        rng = np.random.default_rng(case.seed + 99)
        if case.lattice == "L0":
            wt = EL.ints(rng, (cout, 2 * s, case.K), 8, -4)
        else:
            wt = EL.two_level(rng, (cout, 2 * s, case.K), 128, -3, case.density)
        inp["w"] = _convT_to_gemm(np.ascontiguousarray(wt.transpose(2, 0, 1)), s)          # [s cout][3][cin]
        inp["bias"] = np.tile(inp["bias"][:cout], s)
        inp["up"] = (s, cout)
    return inp


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# launching
_KEEP = []


def dev(a):
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _KEEP.append(t)
    return t


def _slack_rows(t, M):
    """the PAD rows on both sides of a plane ([rows][..] or [chunks][rows][4])"""
    return torch.cat([t[:PAD], t[PAD + M:]]) if t.dim() == 2 else torch.cat([t[:, :PAD], t[:, PAD + M:]], 1)


def _guarded(M, N, dtype):
    """[PAD + M + PAD][N] output filled with a sentinel: the guard rows must survive"""
    return torch.full((M + 2 * PAD, N), SENT, device="cuda", dtype=dtype)


def _host_planes(a):
    """a [R][C] fp32 (R = M + 2 PAD) -> _PlaneSet holding the host quantiser's planes of a"""
    R, Cc = a.shape
    h16, ch, cl, sh, sl = EL.plane_set(a)
    ps = _PlaneSet(R - 2 * PAD, Cc)
    ps.h.copy_(torch.from_numpy(h16))
    for i, (codes, sb) in enumerate(((ch, sh), (cl, sl))):
        ps.q4[i].copy_(torch.from_numpy(np.ascontiguousarray(codes)))
        if Cc == 64:
            sb4 = np.concatenate([sb, np.ones((R, 2), np.uint8)], 1)[None]
        else:
            sb4 = np.ascontiguousarray(sb.reshape(R, Cc // 128, 4).transpose(1, 0, 2))
        ps.qs[i].copy_(torch.from_numpy(sb4))
    return ps


def _mxo_slope(case):
    """the consumer's slope of an emitted plane set (a partial set holds raw values)"""
    return 1.0 if "partial" in case.extra else (0.5 if "up4" in case.extra else 0.125)


def build_desc(lib, case, inp, ps_in=None):
    """-> (descriptor, dict of the output buffers)"""
    from emotivoice_amd import _ffi, mxfp4
    M, K, N, taps = case.M, case.K, case.N, case.taps
    d = _ffi.ev_conv_gemm_desc()
    d.dtype = case.dtype
    w = inp["w"]
    hi = w.astype(np.float16)
    if case.dtype == 0:
        x = dev(inp["x"].astype(np.float16))
        d.W = dev(hi).data_ptr()
    else:
        x = dev(inp["x"])
        if case.dtype == 1:
            d.W = dev(w).data_ptr()
        else:
            d.W, d.W_lo = dev(hi).data_ptr(), dev(((w - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)).data_ptr()
    outs = {}
    if case.dtype == 3:
        d.W_mx = dev(mxfp4.pack_c64_weight_planes(w) if K == 64 else mxfp4.pack_weight_planes(w)).data_ptr()
        if "planes_in" in case.extra:
            ps = _host_planes(inp["x"]) if ps_in is None else ps_in
            _KEEP.append(ps)
            ps.in_fields(d)
            outs["ps_in"] = ps
        else:
            nb = lib.ev_op_mx_scratch_bytes(M, K)
            scratch = torch.zeros(nb, dtype=torch.uint8, device="cuda")
            _KEEP.append(scratch)
            d.mx_scratch, d.mx_scratch_size = scratch.data_ptr(), nb
    if "planes_in" not in case.extra:
        d.A, d.lda = x[PAD:].data_ptr(), K
    d.M, d.N, d.K, d.taps, d.dil, d.center = M, N, K, taps, case.dil, case.center
    d.out_scale = case.scale if case.has("scale") else 1.0
    if case.has("bias"):
        d.bias = dev(inp["bias"]).data_ptr()
    if case.mask:
        d.row_valid, d.valid_shift = dev(inp["valid"]).data_ptr(), case.mask
    if case.has("seq_bias"):
        d.row_seq, d.seq_bias, d.ld_seq_bias = dev(inp["row_seq"]).data_ptr(), dev(inp["seq_bias"]).data_ptr(), N
    if case.has("relu"):
        d.act = 1
    if case.has("lrelu"):
        d.act, d.act_slope = 3, case.slope
    if case.has("pro"):
        d.pro_lrelu, d.pro_slope = 1, case.slope
    if case.has("res16") or case.has("res32"):
        d.res, d.res_dtype, d.ldres = dev(inp["res"]).data_ptr(), (0 if inp["res"].dtype == np.float16 else 1), N
    if case.has("acc32"):
        d.acc32, d.ldacc = dev(inp["acc32"]).data_ptr(), N
    if case.has("respl"):          # the residual from the plane set of lrelu(residual, slope): fp16 hi plane + the remainder's codes and scales
        ps_r = _host_planes(inp["respl"])
        _KEEP.append(ps_r)
        d.res, d.res_dtype, d.ldres = ps_r.h[PAD:].data_ptr(), 3, N
        d.res_x4, d.res_xs, d.res_xs_stride, d.res_inv_slope = ps_r.q4[1][PAD:].data_ptr(), ps_r.qs[1][0, PAD:].data_ptr(), ps_r.R * 4, 1.0 / case.slope
    if case.has("accpl"):          # the running sum as a partial plane set
        ps_s = _host_planes(inp["accpl"])
        _KEEP.append(ps_s)
        d.acc_h, d.acc_x4, d.acc_xs, d.acc_xs_stride, d.ldacc = ps_s.h[PAD:].data_ptr(), ps_s.q4[1][PAD:].data_ptr(), ps_s.qs[1][0, PAD:].data_ptr(), ps_s.R * 4, N
    if case.has("add16"):
        d.add16_a, d.add16_b, d.ldadd = dev(inp["add16"][0]).data_ptr(), dev(inp["add16"][1]).data_ptr(), N
    if case.has("post"):
        d.post_lrelu, d.post_slope = 1, case.slope
    d.out32_before_post = 1 if case.has("before_post") else 0
    if case.outs in ("16", "both"):
        outs["out16"] = _guarded(M, N, torch.float16)
        d.out16 = outs["out16"][PAD:].data_ptr()
    if case.outs in ("32", "both"):
        outs["out32"] = _guarded(M, N, torch.float32)
        d.out32 = outs["out32"][PAD:].data_ptr()
    d.ldo = N
    if "mxo" in case.extra:
        s, cout = inp.get("up", (1, N))
        ps_o = _PlaneSet(M * s, cout)
        if "inplace" in case.extra:          # the second ResBlock rewrites the partial it adds: sentinels where a partial set has no planes
            ps_o = ps_s
            ps_o.q4[0].fill_(0x77)
            ps_o.qs[0].fill_(130)
            outs["slack"] = [(t, _slack_rows(t, M).clone()) for t in (ps_o.h, ps_o.q4[1], ps_o.qs[1])]
        ps_o.out_fields(d, _mxo_slope(case))
        d.mxo_partial = 1 if "partial" in case.extra else 0
        outs["ps_out"] = ps_o
    if "up" in inp:
        d.polyphase_cout = inp["up"][1]
    r0 = [e for e in case.extra if e.startswith("r0=")]
    d.reserved0 = case.dbg | (int(r0[0][3:]) if r0 else 0)
    if case.ksplit:
        ws = torch.zeros(case.ksplit * M * N + 4, dtype=torch.float32, device="cuda")
        _KEEP.append(ws)
        d.ksplit, d.mx_scratch, d.mx_scratch_size = case.ksplit, ws.data_ptr(), case.ksplit * M * N * 4
    return d, outs


def _sync_or_stop(what):
    """a device fault ends the session: nothing more is launched on a card that has faulted"""
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:
        pytest.exit("device fault in %s: %s" % (what, e), returncode=3)


def launch(lib, case, inp, dbg=0, ps_in=None):
    d, outs = build_desc(lib, case, inp, ps_in)
    d.reserved0 |= dbg
    torch.cuda.synchronize()
    rc = lib.ev_op_conv_gemm(C.byref(d), None)
    _sync_or_stop(case.name)
    assert rc == 0, (case.name, rc)
    return outs


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# references
def _is_long(case):
    return 2.0 * case.M * case.N * case.K * case.taps > LONG_FLOP


def _sample_rows(case):
    """a few hundred rows of a long case: both ends, one 256-row tile edge, the edge of a masked run if there is one, a random sample"""
    M = case.M
    r = [np.arange(0, 64), np.arange(M - 64, M), np.arange(256 - 32, 256 + 32), np.random.default_rng(1).integers(0, M, 128)]
    for first, n in case.mask_runs:
        r.append(np.arange(max(0, (first << case.mask) - 16), min(M, ((first + n) << case.mask) + 16)))
    return np.unique(np.concatenate(r))


def expected_device(case, inp):
    """EL.expected on the device in torch fp64: -> (out32 value, out16 / plane value) as [M][N] fp64 tensors"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda().double()          # noqa: E731
    M = case.M
    v = torch.zeros(M, case.N, dtype=torch.float64, device="cuda")
    for xp, wp in EL.operand_parts(case, inp):
        xd, wd = t(xp), t(wp)
        for tap in range(case.taps):
            o = PAD + (tap - case.center) * case.dil
            v += xd[o:o + M] @ wd[:, tap, :].T
        del xd, wd
    lr = lambda z: torch.where(z > 0, z, z * case.slope)          # noqa: E731
    if case.has("bias"):
        v += t(inp["bias"])
    if case.has("relu"):
        v = v.clamp(min=0)
    if case.has("lrelu"):
        v = lr(v)
    if case.has("seq_bias"):
        v += t(inp["seq_bias"])[torch.from_numpy(inp["row_seq"]).cuda().long()]
    if case.has("res16") or case.has("res32"):
        v += t(inp["res"])
    if case.has("scale"):
        v *= case.scale
    if case.has("acc32"):
        v += t(inp["acc32"])
    if case.has("add16"):
        v += t(inp["add16"][0])
        v += t(inp["add16"][1])
    post = lr(v) if case.has("post") else v
    if case.mask:
        m = torch.from_numpy(inp["vrow"]).cuda()[:, None]
        v, post = v * m, post * m
    return (v if case.has("before_post") else post), post


def reference(case, inp):
    """-> dict(out32 =, out16 =, exact =): numpy arrays (short cases, CPU) or device tensors (long cases, after the sampled rows agreed with the CPU evaluation)"""
    if not _is_long(case):
        return EL.expected(case, inp)
    v32, v16 = expected_device(case, inp)
    rows = _sample_rows(case)
    want = EL.expected(case, inp, rows)
    ridx = torch.from_numpy(rows).cuda()
    EL.compare(v32[ridx].cpu().numpy(), want["out32"], what=case.name + ": device reference, out32 rows")
    EL.compare(v16[ridx].cpu().numpy(), want["exact"], what=case.name + ": device reference, out16 rows")
    assert bool((v32.float().double() == v32).all())
    return dict(out32=v32.float(), out16=v16.half(), exact=v16)


def count_mismatches(got, want, kind="value"):
    """got: device tensor [rows][cols]; want: numpy array or device tensor -> (count, message)"""
    if isinstance(want, torch.Tensor):
        bad = ~(torch.isfinite(got) & (got.double() == want.double()))
        n = int(bad.sum())
        if n == 0:
            return 0, ""
        return EL.mismatches(got.float().cpu().numpy(), want.float().cpu().numpy())
    return EL.mismatches(got.cpu().numpy(), want, kind)


def _guards_ok(buf, M):
    return bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + M:] == SENT).all())


def check_outputs(case, inp, outs, ref, tag=""):
    """every output of a launch against the reference, element by element -> (elements compared, mismatches); asserts zero mismatches"""
    M = case.M
    n_el, n_bad, msgs = 0, 0, []
    for name in ("out32", "out16"):
        if name in outs:
            assert _guards_ok(outs[name], M), (case.name, name, "guard rows written")
            n, msg = count_mismatches(outs[name][PAD:PAD + M], ref[name])
            n_el += M * case.N
            n_bad += n
            if n:
                msgs.append("%s%s %s: %s" % (case.name, tag, name, msg))
    if "ps_out" in outs:
        ps = outs["ps_out"]
        s, cout = inp.get("up", (1, case.N))
        Mo = M * s
        exact = ref["exact"]
        exact = exact.cpu().numpy() if isinstance(exact, torch.Tensor) else exact
        h16, ch, cl, sh, sl = EL.plane_set(exact.reshape(Mo, cout), _mxo_slope(case))
        partial = "partial" in case.extra
        if "slack" in outs:          # in place: the slack rows keep what they held
            assert all(torch.equal(_slack_rows(t, Mo), before) for t, before in outs["slack"]), (case.name, "plane slack rows written")
        else:
            assert bool((ps.h[:PAD] == 3.0).all()) and bool((ps.h[PAD + Mo:] == 3.0).all())
        planes = [("h", ps.h[PAD:PAD + Mo], h16, "value")]
        for i, (codes, sb) in enumerate(((ch, sh), (cl, sl))):
            if partial and i == 0:          # a partial set has no hi-code plane: those buffers are not written
                assert bool((ps.q4[0] == 0x77).all()) and bool((ps.qs[0] == 130).all()), (case.name, "hi codes / scales of a partial set written")
                continue
            if "slack" not in outs:
                assert bool((ps.q4[i][:PAD] == 0x77).all()) and bool((ps.q4[i][PAD + Mo:] == 0x77).all()) and bool((ps.qs[i][:, :PAD] == 130).all()) and \
                    bool((ps.qs[i][:, PAD + Mo:] == 130).all()), (case.name, "plane slack rows written")
            planes.append(("q4[%d]" % i, ps.q4[i][PAD:PAD + Mo], codes, "codes"))
            if cout == 64:
                got_s = ps.qs[i][0, PAD:PAD + Mo, :2]
            else:
                got_s = ps.qs[i][:, PAD:PAD + Mo].permute(1, 0, 2).reshape(Mo, cout // 32)
            planes.append(("qs[%d]" % i, got_s, sb, "bytes"))
        for pname, got, want, kind in planes:
            n, msg = count_mismatches(got, want, kind)
            n_el += int(np.asarray(want).size)
            n_bad += n
            if n:
                msgs.append("%s%s plane %s: %s" % (case.name, tag, pname, msg))
    return n_el, n_bad, msgs


def _record(case, bits, n_el, n_bad, key=None):
    write_report(key or case.name, dict(kernel=case.kernel, shape=dict(M=case.M, K=case.K, N=case.N, taps=case.taps, dil=case.dil), lattice=case.lattice,
                                        budget_bits=round(bits, 2), elements=n_el, mismatches=n_bad), "exact_report.json", REPORT)


def run_case(lib, case, dbgs=(0,)):
    inp = case_inputs(case)
    bits = EL.budget(case, inp)
    assert bits < EL.LIMIT_BITS, (case.name, bits)          # the precondition: checked before anything is launched
    ref = reference(case, inp)
    for dbg in dbgs:
        outs = launch(lib, case, inp, dbg)
        n_el, n_bad, msgs = check_outputs(case, inp, outs, ref, " reserved0=%d" % dbg if dbg else "")
        _record(case, bits, n_el, n_bad, case.name + (":reserved0=%d" % dbg if dbg else ""))
        assert n_bad == 0, "\n".join(msgs)
        del outs
    del _KEEP[:]
    return inp, ref


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# the tests
@pytest.mark.parametrize("case", F16_TILE_CASES, ids=_ids(F16_TILE_CASES))
def test_exact_f16_tiles(lib, case):
    """conv_gemm_kernel<_Float16> in its <256,32>, <256,64>, latency <256,32>, <128,128> and <256,128> configurations: out32 exact, out16 its RNE"""
    run_case(lib, case)


@pytest.mark.parametrize("case", F16_EPI_CASES, ids=_ids(F16_EPI_CASES))
def test_exact_f16_epilogues(lib, case):
    """every straight-line fp16 epilogue of launch_cfg and the generic one, row masks at valid_shift 3 across a 256-row tile edge"""
    run_case(lib, case)


@pytest.mark.parametrize("case", PHASED_CASES, ids=_ids(PHASED_CASES))
def test_exact_phased(lib, case):
    """conv_gemm_phased_kernel (taps 3 / 7 / 11 at BN 128, 11 at BN 64; five epilogue variants) and, with reserved0 bit 2, the 4-wave kernel on the same launch"""
    run_case(lib, case, dbgs=(0, 4))


@pytest.mark.parametrize("case", F32_CASES, ids=_ids(F32_CASES))
def test_exact_f32(lib, case):
    """conv_gemm_kernel<float>: the four tile configurations (<256,128> from 2048 tiles on)"""
    run_case(lib, case)


@pytest.mark.parametrize("case", X3_CASES, ids=_ids(X3_CASES))
def test_exact_split_precision(lib, case):
    """conv_gemm_split_kernel, conv_gemm_x3_kernel at BN 128 / 64 / 32 and split-K + splitk_reduce_kernel on L0 (hi pass, indexing, epilogues) and L1 (the cross terms)"""
    run_case(lib, case)


@pytest.mark.parametrize("case", MX_CASES, ids=_ids(MX_CASES))
def test_exact_mx(lib, case):
    """the MX kernels: fp32 input through mx_planes_kernel and plane-set input from the host quantiser; emitted plane sets byte for byte against mxfp4.py on the
    exact value (code 8 == code 0), slack rows untouched"""
    run_case(lib, case)


@pytest.mark.parametrize("lat", ["L0", "L1"])
def test_exact_mx_input_forms_agree(lib, lat):
    """the same problem with fp32 input (mx_planes_kernel) and with the host quantiser's plane set: the same (exact) bits"""
    base = [c for c in MX_CASES if c.name == "mx_%s_k7_res32_mxo" % lat][0]
    inp = case_inputs(base)
    assert EL.budget(base, inp) < EL.LIMIT_BITS
    a = launch(lib, base, inp)
    import dataclasses
    b = launch(lib, dataclasses.replace(base, extra=("mxo", "planes_in")), inp)
    assert torch.equal(a["out32"], b["out32"]) and torch.equal(a["ps_out"].h, b["ps_out"].h)
    del _KEEP[:]


@pytest.mark.parametrize("triple", GROUP3_CASES, ids=[t[0].name[3:-4] for t in GROUP3_CASES])
def test_exact_mx_group3(lib, triple):
    """ev_op_conv_gemm_group3 on an engine triple (11 / 7 / 3 taps, one input plane set, planes only out): each member's plane set against mxfp4.py on its exact value"""
    from emotivoice_amd import _ffi
    inp0 = case_inputs(triple[0])
    ps_in = _host_planes(inp0["x"])
    arr = (_ffi.ev_conv_gemm_desc * 3)()
    members = []
    for i, case in enumerate(triple):
        inp = case_inputs(case)
        inp["x"], inp["valid"], inp["vrow"] = inp0["x"], inp0["valid"], inp0["vrow"]          # one activation (and residual) for all three
        if case.has("respl"):
            inp["respl"] = inp0["respl"]
        bits = EL.budget(case, inp)
        assert bits < EL.LIMIT_BITS, (case.name, bits)
        d, outs = build_desc(lib, case, inp, ps_in)
        C.memmove(C.byref(arr[i]), C.byref(d), C.sizeof(d))
        members.append((case, inp, outs, bits))
    torch.cuda.synchronize()
    assert lib.ev_op_conv_gemm_group3(arr, 0, None) == 0
    _sync_or_stop("group3")
    for case, inp, outs, bits in members:
        n_el, n_bad, msgs = check_outputs(case, inp, outs, EL.expected(case, inp))
        _record(case, bits, n_el, n_bad)
        assert n_bad == 0, "\n".join(msgs)
    del _KEEP[:]


@pytest.mark.parametrize("case", NEGATIVE_CASES, ids=_ids(NEGATIVE_CASES))
def test_negative_controls(lib, case):
    """a passing launch against the reference of a deliberately different problem: every one must be reported as mismatches"""
    inp = case_inputs(case)
    outs = launch(lib, case, inp)
    got = outs["out32"][PAD:PAD + case.M].cpu().numpy()
    assert EL.mismatches(got, EL.expected(case, inp)["out32"])[0] == 0
    found = {}
    if (case.taps - 1) * (case.dil + 1) <= 64:
        found["dil+1"] = EL.mismatches(got, EL.expected(case, inp, dil=case.dil + 1)["out32"])[0]
    found["center-1"] = EL.mismatches(got, EL.expected(case, inp, center=case.center - 1)["out32"])[0]
    w2 = inp["w"].copy()
    w2[:, [0, case.taps - 1]] = w2[:, [case.taps - 1, 0]]
    found["taps swapped"] = EL.mismatches(got, EL.expected(case, inp, w=w2)["out32"])[0]
    if case.lattice == "L1":          # the cross terms are in play: the hi pass alone is not the answer
        found["lo parts of w dropped"] = EL.mismatches(got, EL.expected(case, inp, w=inp["w"].astype(np.float16).astype(np.float32))["out32"])[0]
    if "planes_in" in case.extra:
        ps = _host_planes(inp["x"])
        r, blk = PAD + case.M // 2 + 3, 1
        assert inp["vrow"][case.M // 2 + 3] and inp["x"][r, 32 * blk:32 * blk + 32].any()
        ps.qs[0][0, r, blk] += 1          # the hi operand's scale of one 32-channel block of one row
        ps.qs[1][0, r, blk] += 1
        got2 = launch(lib, case, inp, ps_in=ps)["out32"][PAD:PAD + case.M].cpu().numpy()
        found["scale byte"] = EL.mismatches(got2, EL.expected(case, inp)["out32"])[0]
    write_report("negative:" + case.name, found, "exact_report.json", REPORT)
    assert all(v > 0 for v in found.values()), (case.name, found)
    del _KEEP[:]


# ---------------------------------------------------------------------------------------------------------------------------------------------------
# Fused ResBlock pairs, lattice L0, through the harness classes of test_gpu_pair_long.py (their launch code; the inputs are replaced by lattice tensors).
# The pair kernels fix their leaky-relu slope at 0.1, which is not dyadic: the inputs are therefore chosen so that no leaky-relu ever sees a negative value
# (x >= 0; b1 >= the largest negative sum conv1 can reach, so the intermediate is >= 0 with signed weights).  That is a restriction of the inputs, stated
# here, not a tolerance: indexing, halos, masks, tile hand-over, the fp16 / split storage of the intermediate and the epilogue are all held exactly.  The
# harness's out_scale (1/3) and post slope (0.01) are replaced by dyadic ones on the way to the entry point.  The intermediate is modelled as the kernel
# stores it: fp16 round-to-nearest-even (fp16 pairs), the host split and quantiser of the exact value (MX pairs: mxfp4.quantize / e5m2_*).
PAIR_CASES = [
    # name, kernel, harness, C, k, dil, form, segments per 256 CUs
    ("pair_c32_k3_d5_add16", "resblock_pair_c32_kernel<3,2,false>", "f16", 32, 3, 5, "add16", 68),
    ("pair_c32_k3_d1_twob_acc32", "resblock_pair_c32_kernel<3,1,true> (two blocks per CU) and, reserved0 bit 2, one block", "f16", 32, 3, 1, "acc32", 258),
    ("pair_c32_k7_d3_acc32", "resblock_pair_c32_kernel<7,1,false>", "f16", 32, 7, 3, "acc32", 68),
    ("pair_c32_k11_d5_none", "resblock_pair_c32_kernel<11,0,false>", "f16", 32, 11, 5, "none", 68),
    ("pair_c32_k11_d1_add16", "resblock_pair_c32_kernel<11,2,false>", "f16", 32, 11, 1, "add16", 68),
    ("pair_c64_k3_d1_none", "resblock_pair_c64_kernel<3,0>", "f16", 64, 3, 1, "none", 68),
    ("pair_c64_k3_d3_acc32", "resblock_pair_c64_kernel<3,1>", "f16", 64, 3, 3, "acc32", 68),
    ("pair_c64_k3_d5_add16", "resblock_pair_c64_kernel<3,2>", "f16", 64, 3, 5, "add16", 68),
    ("pair_mx_c32_k3_d5_acc", "resblock_pair_c32_e5_kernel / _mx2_kernel / _mx_kernel <3>", "mx32", 32, 3, 5, "acc", 68),
    ("pair_mx_c32_k7_d1", "resblock_pair_c32_e5_kernel / _mx2_kernel / _mx_kernel <7>", "mx32", 32, 7, 1, "none", 68),
    ("pair_mx_c32_k11_d5_acc", "resblock_pair_c32_e5_kernel / _mx2_kernel / _mx_kernel <11>", "mx32", 32, 11, 5, "acc", 68),
    ("pair_mx_c64_d1_planes", "resblock_pair_c64_mx_kernel<false>", "mx64", 64, 3, 1, "planes", 68),
    ("pair_mx_c64_d5_acc_o32_planes", "resblock_pair_c64_mx_kernel<true>", "mx64", 64, 3, 5, "acc+o32+planes", 68),
    ("pair_mx_c64_d3_o32", "resblock_pair_c64_mx_kernel<false>", "mx64", 64, 3, 3, "o32", 68),
]
# The cross terms of the MX pairs, on L1 with a ROUTING conv on the other side (one nonzero weight per output channel, a power of two at a random tap and
# input channel: its output stays on the lattice and its sum has one term).  route "conv2": two-level x (>= 0) and w1 on conv1, whose arbitrary fp32
# result is split and quantised as the host does, routed by conv2; route "conv1": conv1 routes the two-level x (xt = x / 2, on the lattice), conv2 has a
# two-level w2.  The last field is the L1 density.
PAIR_CASES += [
    ("pair_mx_c32_k3_d1_route2", "resblock_pair_c32_e5 / _mx2 / _mx <3>, L1 conv1, routing conv2", "mx32", 32, 3, 1, "acc", 68, "conv2", 0.3),
    ("pair_mx_c32_k7_d3_route2", "resblock_pair_c32_e5 / _mx2 / _mx <7>, L1 conv1, routing conv2", "mx32", 32, 7, 3, "none", 68, "conv2", 0.14),
    ("pair_mx_c32_k11_d5_route1", "resblock_pair_c32_e5 / _mx2 / _mx <11>, routing conv1, L1 conv2", "mx32", 32, 11, 5, "acc", 68, "conv1", 0.25),
    ("pair_mx_c32_k3_d5_route1", "resblock_pair_c32_e5 / _mx2 / _mx <3>, routing conv1, L1 conv2", "mx32", 32, 3, 5, "none", 68, "conv1", 0.5),
    ("pair_mx_c64_d3_route2", "resblock_pair_c64_mx_kernel, L1 conv1, routing conv2", "mx64", 64, 3, 3, "acc+o32+planes", 68, "conv2", 0.2),
    ("pair_mx_c64_d1_route1", "resblock_pair_c64_mx_kernel, routing conv1, L1 conv2", "mx64", 64, 3, 1, "o32+planes", 68, "conv1", 0.4),
]
PAIR_SCALE, PAIR_POST, PAIR_MXO_SLOPE = 0.5, 0.125, 0.125


def routing(rng, Cc, k, exps, signed):
    """[C][k][C] with one nonzero weight per output channel: a (signed) power of two at a random tap and input channel"""
    w = np.zeros((Cc, k, Cc), np.float32)
    n = np.arange(Cc)
    sgn = rng.choice(np.array([-1.0, 1.0]), Cc) if signed else 1.0
    w[n, rng.integers(0, k, Cc), rng.integers(0, Cc, Cc)] = np.ldexp(sgn, rng.choice(np.asarray(exps), Cc)).astype(np.float32)
    return w


def pair_layout(S, seed=2024):
    """S segments at a pitch of 1024 rows, valid lengths 600 .. 992 in steps of 8, three segments entirely invalid (all-gap tiles), the last one ending 40 rows
    short of M -> [M] bool"""
    rng = np.random.default_rng(seed)
    lens = 600 + 8 * rng.integers(0, 50, S)
    lens[S // 3:S // 3 + 3] = 0
    lens[-1] = 984
    return (np.arange(1024)[None, :] < lens[:, None]).reshape(-1)


def pair_inputs(pc, n_cu=256):
    name, kernel, harness, Cc, k, dil, form, seg = pc[:8]
    route, dens = pc[8:] if len(pc) > 8 else (None, 1.0)
    vrow = pair_layout(max(8, seg * n_cu // 256))
    M = vrow.size
    rng = np.random.default_rng(len(name) * 31 + k + dil)
    xq = {3: -4, 7: -3, 11: -2}[k] + (1 if Cc == 64 else 0)
    x = np.zeros((M + 2 * PAD, Cc), np.float32)
    x[PAD:PAD + M] = np.ldexp(rng.integers(0, (1 << -xq) + 1, (M, Cc)).astype(np.float32), xq) * vrow[:, None]          # 0 .. 1
    w1, w2 = EL.ints(rng, (Cc, k, Cc), 4, -4), EL.ints(rng, (Cc, k, Cc), 4, -4)
    b1 = (np.maximum(-w1, 0).sum((1, 2)) + EL.ints(rng, (Cc,), 8, -4).clip(0)).astype(np.float32)          # conv1 + b1 >= 0 for every x in [0, 1]
    b2 = EL.ints(rng, (Cc,), 64, -6)
    if route:
        x[PAD:PAD + M] = np.abs(EL.two_level(rng, (M, Cc), 32, -2, dens)) * vrow[:, None]          # < 2
        b2 = EL.ints(rng, (Cc,), 16, -6)
        if route == "conv2":
            w1, w2 = EL.two_level(rng, (Cc, k, Cc), 32, -3, dens), routing(rng, Cc, k, (-1, 0), True)
            w1 = np.where((w1 < 0) & (rng.random(w1.shape) < 0.75), -w1, w1)          # an eighth negative: b1, and with it the intermediate's magnitude, stays small
            b1 = (2.0 * np.maximum(-w1.astype(np.float64), 0).sum((1, 2))).astype(np.float32)          # conv1 + b1 >= 0 for every x in [0, 2)
            assert np.array_equal(b1.astype(np.float64), 2.0 * np.maximum(-w1.astype(np.float64), 0).sum((1, 2)))
        else:
            w1, w2 = routing(rng, Cc, k, (-1,), False), EL.two_level(rng, (Cc, k, Cc), 32, -3, dens)
            b1 = np.zeros(Cc, np.float32)
    p = dict(name=name, kernel=kernel, harness=harness, C=Cc, k=k, dil=dil, form=form, M=M, vrow=vrow, x=x, w1=w1, w2=w2, b1=b1, b2=b2, lattice="L1" if route else "L0")
    if "acc" in form:
        p["acc"] = EL.ints(rng, (M, Cc), 1023 if not route else 255, -8)
    if form == "add16":
        p["add16"] = (EL.ints(rng, (M, Cc), 255, -6).astype(np.float16), EL.ints(rng, (M, Cc), 255, -6).astype(np.float16))
    return p


def _act_parts(a, fmt):
    """the operands a kernel of format fmt makes of an activation a (numpy fp32): [(activation part, index of the weight part it multiplies)]"""
    from emotivoice_amd import mxfp4
    if fmt == "f16":
        assert np.array_equal(a.astype(np.float16).astype(np.float32), a)
        return [(a, 0)]
    hi, lo = mxfp4.split_hi_lo(a)
    if fmt == "e5m2":
        return [(hi, 0), (mxfp4.e5m2_decode(mxfp4.e5m2_hi_codes(hi)), 1), (mxfp4.e5m2_lo_decode(mxfp4.e5m2_lo_codes(lo)), 2)]
    q = lambda v: mxfp4.dequantize(*mxfp4.quantize(v, 32), 32)          # noqa: E731
    return [(hi, 0), (q(hi), 1), (q(lo), 2)]


def _w_parts(w, fmt):
    from emotivoice_amd import mxfp4
    if fmt == "f16":
        return [w]
    hi, lo = mxfp4.split_hi_lo(w)
    q = lambda v: mxfp4.dequantize(*mxfp4.quantize(v, 32, mxfp4.W_RULE), 32)          # noqa: E731
    return [hi, q(lo), q(hi)]


def pair_reference(p, fmt, device):
    """the pair in torch fp64 on ``device`` -> (value before the post leaky-relu [M][C] (out32), value after it (out16 / planes), budget bits of the worse conv)"""
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(device).double()          # noqa: E731
    M, k, dil, h2 = p["M"], p["k"], p["dil"], (p["k"] - 1) // 2
    vpad = np.zeros(M + 2 * PAD, bool)
    vpad[PAD:PAD + M] = p["vrow"]

    def conv(acts, ws, n_rows, first, step):
        """rows first .. first + n_rows of sum_parts sum_t a[. + (t - h2) step] @ w_t.T, and the same on magnitudes with the smallest product quantum"""
        v = torch.zeros(n_rows, p["C"], dtype=torch.float64, device=device)
        mag, q = torch.zeros_like(v), np.inf
        for a, wi in acts:
            w = ws[wi]
            if not a.any() or not w.any():
                continue
            q = min(q, EL.quantum(a) * EL.quantum(w))
            ad, wd = t(a), t(w)
            for tap in range(k):
                o = first + (tap - h2) * step
                v += ad[o:o + n_rows] @ wd[:, tap, :].T
                mag += ad[o:o + n_rows].abs() @ wd[:, tap, :].abs().T
        return v, mag, q

    # conv1 on rows -h2 .. M + h2 (what conv2 reads), bias, leaky-relu (never active), sequence-edge mask
    x = p["x"]
    n1 = M + 2 * h2
    c1, mag1, q1 = conv(_act_parts(x, fmt), _w_parts(p["w1"], fmt), n1, PAD - h2, dil)
    c1 += t(p["b1"])
    bits1 = float(torch.log2((mag1 + t(p["b1"]).abs()).max() / min(q1, EL.quantum(p["b1"]))))
    p["cross1"] = sum(1 for a, wi in _act_parts(x, fmt) if a.any() and _w_parts(p["w1"], fmt)[wi].any()) if fmt != "f16" else 1
    assert float(c1.min()) >= 0.0          # the fixed slope 0.1 never acts
    c1 *= t(vpad[PAD - h2:PAD - h2 + n1].astype(np.float64))[:, None]
    xt = c1.float()
    assert bool((xt.double() == c1).all())
    xt = xt.cpu().numpy()
    if fmt == "f16":
        xt = xt.astype(np.float16).astype(np.float32)          # the intermediate lives in LDS as fp16 (round to nearest even)
    y, mag2, q2 = conv(_act_parts(xt, fmt), _w_parts(p["w2"], fmt), M, h2, 1)
    xres = t(x[PAD:PAD + M])
    y = (y + t(p["b2"]) + xres) * PAIR_SCALE
    mag2 = (mag2 + t(p["b2"]).abs() + xres) * PAIR_SCALE
    q2 = min(q2, EL.quantum(p["b2"]), EL.quantum(x)) * PAIR_SCALE
    for add in ([p["acc"]] if "acc" in p else []) + list(p.get("add16", ())):
        y += t(add)
        mag2 += t(add).abs()
        q2 = min(q2, EL.quantum(add))
    bits2 = float(torch.log2(mag2.max() / q2))          # (the post leaky-relu multiplies by a power of two and nothing is added after it)
    m = t(p["vrow"].astype(np.float64))[:, None]
    post = torch.where(y > 0, y, y * (PAIR_MXO_SLOPE if p["harness"] == "mx64" else PAIR_POST))
    return y * m, post * m, max(bits1, bits2)


class _DyadicLib:
    """the library with the pair entry points' out_scale / post slope replaced by dyadic ones (the harness classes fix 1/3 and 0.01)"""

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if not name.startswith("ev_op_resblock_pair"):
            return fn

        def call(ref, stream):
            e = ref._obj.epi
            e.out_scale = PAIR_SCALE
            if e.post_lrelu:
                e.post_slope = PAIR_POST
            return fn(ref, stream)
        return call


class _L:
    """what the harness classes read of a layout"""

    def __init__(self, p):
        self.M, self.vrow = p["M"], torch.from_numpy(p["vrow"])
        self.vrow_d = self.vrow.cuda()
        self.valid = torch.from_numpy(p["vrow"].reshape(-1, 8)[:, 0].astype(np.uint8)).cuda()


def _pair_check(p, key, got, want, bits, kind="value"):
    n, msg = count_mismatches(got, want, kind)
    write_report(key, dict(kernel=p["kernel"], shape=dict(M=p["M"], C=p["C"], k=p["k"], dil=p["dil"]), lattice=p["lattice"], budget_bits=round(bits, 2),
                           elements=int(got.numel()), mismatches=n), "exact_report.json", REPORT)
    assert n == 0, "%s: %s" % (key, msg)


def _guard(buf, M, sent=SENT):
    assert bool((buf[:PAD] == sent).all()) and bool((buf[PAD + M:] == sent).all()), "guard rows written"


@pytest.mark.parametrize("pc", PAIR_CASES, ids=[c[0] for c in PAIR_CASES])
def test_exact_pairs(lib, pc):
    """every fused pair kernel at more than one tile per block: out32 / out16 / the emitted plane set element by element"""
    import test_gpu_pair_long as PL
    from emotivoice_amd import mxfp4
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    p = pair_inputs(pc, n_cu)
    name, harness, Cc, k, dil, form, M = p["name"], p["harness"], p["C"], p["k"], p["dil"], p["form"], p["M"]
    assert PL.VSHIFT == 3 and PL.PAD == PAD
    L, dlib = _L(p), _DyadicLib(lib)
    h2 = (k - 1) // 2
    hw = lambda w: torch.from_numpy(w.astype(np.float16)).cuda()          # noqa: E731
    if harness == "f16":
        bmo = 256 - 2 * h2
        ntiles = -(-M // bmo)
        twob = "twob" in name
        assert (Cc == 32 and k == 3 and ntiles >= 4 * n_cu) == twob and ntiles > (2 * n_cu if twob else n_cu)          # the launcher's rule; > 1 tile per block
        v32, v16, bits = pair_reference(p, "f16", "cuda")
        assert bits < EL.LIMIT_BITS, (name, bits)
        P = PL._F16Pair(dlib, L, Cc, k, dil, form, 1)
        P.full = torch.from_numpy(p["x"].astype(np.float16)).cuda()
        P.x = P.full[PAD:PAD + M]
        P.w1g, P.w2g, P.b1, P.b2 = hw(p["w1"]), hw(p["w2"]), torch.from_numpy(p["b1"]).cuda(), torch.from_numpy(p["b2"]).cuda()
        if form == "acc32":
            P.acc = torch.from_numpy(p["acc"]).cuda()
        if form == "add16":
            P.a16, P.b16 = torch.from_numpy(p["add16"][0]).cuda(), torch.from_numpy(p["add16"][1]).cuda()
        for r0 in ((0, 4) if twob else (0,)):
            o16, o32 = P.run(P.full, L.valid, 0, M, reserved0=r0)
            _guard(o16, M)
            _guard(o32, M)
            _pair_check(p, "%s:out32:r%d" % (name, r0), o32[PAD:PAD + M], v32.float(), bits)
            _pair_check(p, "%s:out16:r%d" % (name, r0), o16[PAD:PAD + M], v16.half(), bits)
    elif harness == "mx32":
        P = PL._MxPair(dlib, L, k, dil, form == "acc", 1)
        P.full = torch.from_numpy(p["x"]).cuda()
        P.x = P.full[PAD:PAD + M]
        P.b1, P.b2 = torch.from_numpy(p["b1"]).cuda(), torch.from_numpy(p["b2"]).cuda()
        P.w1h, P.w2h = hw(p["w1"]), hw(p["w2"])
        P.w1m, P.w2m = (torch.from_numpy(mxfp4.pack_pair_weight_planes(w)).cuda() for w in (p["w1"], p["w2"]))
        if form == "acc":
            P.acc = torch.from_numpy(p["acc"]).cuda()
        for r0, fmt, gr in ((32, "e5m2", 128), (16, "fp4", 128), (16 | 4, "fp4", 256)):
            assert -(-M // (gr - 2 * h2)) > n_cu * (256 // gr)          # more than one iteration per block
            v32, _, bits = pair_reference(p, fmt, "cuda")
            assert bits < EL.LIMIT_BITS, (name, fmt, bits)
            out = P.run(P.full, L.valid, 0, M, r0)
            _guard(out, M)
            _pair_check(p, "%s:%s:r%d" % (name, fmt, r0), out[PAD:PAD + M], v32.float(), bits)
    else:
        assert -(-M // 126) > n_cu
        v32, vpl, bits = pair_reference(p, "fp4", "cuda")
        assert bits < EL.LIMIT_BITS, (name, bits)
        wset = lambda w: (hw(w), hw((w - w.astype(np.float16).astype(np.float32)) * np.float32(2048.0)), torch.from_numpy(mxfp4.pack_c64_weight_planes(w)).cuda())  # noqa: E731
        inp = dict(L=L, w1=wset(p["w1"]), w2=wset(p["w2"]), b1=torch.from_numpy(p["b1"]).cuda(), b2=torch.from_numpy(p["b2"]).cuda(),
                   acc=torch.from_numpy(p["acc"]).cuda() if "acc" in p else None)
        K = PL._C64Mx(dlib, inp, dil, form, slope=PAIR_MXO_SLOPE)
        out, ps = K.fused(_host_planes(p["x"]), L.valid, 0, M)
        if "o32" in form:
            _guard(out, M)
            _pair_check(p, name + ":out32", out[PAD:PAD + M], v32.float(), bits)
        else:
            assert bool((out == SENT).all())
        if "planes" in form:
            h16, ch, cl, sh, sl = EL.plane_set(vpl.cpu().numpy(), 1.0)          # (vpl already carries the consumer's slope)
            _guard(ps.h, M, 3.0)
            _pair_check(p, name + ":planes:h", ps.h[PAD:PAD + M], h16, bits)
            for i, (codes, sb) in enumerate(((ch, sh), (cl, sl))):
                _guard(ps.q4[i], M, 0x77)
                _pair_check(p, name + ":planes:q4[%d]" % i, ps.q4[i][PAD:PAD + M], codes, bits, "codes")
                _pair_check(p, name + ":planes:qs[%d]" % i, ps.qs[i][0, PAD:PAD + M, :2], sb, bits, "bytes")
        else:
            assert bool((ps.h == 3.0).all())
    del _KEEP[:]
