"""The C-ABI library loads and exports every symbol include/uavgnn.h (the drop-in boundary, and the only header) declares, and the
ctypes table and the UAVGNN_* constants that uav_bs_ctrl_amd/_lib.py reads from that header are what the header says: counted against
the exports, pinned by hand for entries that between them use every type rule, and the parser exercised on a text of its own
(no compute calls without a GPU)."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from uav_bs_ctrl_amd import _lib
from uav_bs_ctrl_amd.build import build_lib


def _declared(root):
    src = open(os.path.join(root, "include", "uavgnn.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(uavgnn_[a-z0-9_]+)\s*\(", src)))


def test_library_builds_loads_and_exports_every_declared_symbol(repo_root):
    path = build_lib()
    assert os.path.exists(path)
    handle = ctypes.CDLL(path)
    names = _declared(repo_root)
    assert not any("_dbg" in n for n in names), "the shipped library carries no debug entries: ablations are side builds of tools/"
    assert "uavgnn_gatv2_fwd" in names and "uavgnn_talk_attn_bwd" in names
    for n in names:
        assert hasattr(handle, n), f"{n} declared in include/uavgnn.h but not exported"
    assert sorted(_lib.SIGNATURES) == names, "ctypes signature table out of sync with the header"
    assert _lib.lib().uavgnn_version() == 101
    assert b"instantiations" in _lib.lib().uavgnn_strerror(-1001)


def test_argument_errors_are_codes_not_crashes():
    L = _lib.lib()
    assert L.uavgnn_gru_gates_fwd(None, None, None, 4, 8, None, None) == -1000
    assert L.uavgnn_gatv2_fwd(None, 0, 4, None, 2, None, None, 3, None, None, None, None, None, None, None, 4, 64, 0.2, None,
                              256, None, None) == -1000
    assert L.uavgnn_gatv2_bwd_workspace_bytes(4, 256) == 1024 * 256 * 12 * 4


def _exported(path):
    """Names of the dynamic uavgnn_* symbols the library DEFINES, from binutils' nm or the ROCm toolchain's llvm-readelf."""
    nm = shutil.which("nm")
    cmd = [nm, "-D", "--defined-only"] if nm else ["/opt/rocm/lib/llvm/bin/llvm-readelf", "--dyn-syms", "-W"]
    out = subprocess.run(cmd + [path], check=True, capture_output=True, text=True).stdout
    return sorted(m[1] for m in re.finditer(r"^(?!.*\bUND\b).*\s(uavgnn_\w+)$", out, re.M))


def test_header_table_and_exports_count_the_same_entries(repo_root):
    names, exported = _declared(repo_root), _exported(build_lib())
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(repo_root, "include", "uavgnn.h")).read(), flags=re.S)
    assert len(re.findall(r"\buavgnn_[a-z0-9_]+\s*\(", src)) == len(names), "an entry point is declared twice"
    assert len(names) == len(_lib.SIGNATURES) == len(exported) == 130
    assert sorted(_lib.SIGNATURES) == names == exported


_I, _F, _D, _LL, _SZ, _P = ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong, ctypes.c_size_t, ctypes.c_void_p
_PP, _PLL = ctypes.POINTER(ctypes.c_void_p), ctypes.POINTER(ctypes.c_longlong)
_PI32, _PD = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double)
# written out from include/uavgnn.h by hand, argument by argument - never by calling the parser
_PINNED = {
    "uavgnn_strerror": (ctypes.c_char_p, [_I]),
    "uavgnn_gatv2_hetero_image_bytes": (_SZ, []),
    #                       t   inc  eps_start eps_end decay_steps eps stream
    "uavgnn_eps_schedule": (_I, [_P, _LL, _D, _D, _D, _P, _P]),
    #                       p g exp_avg exp_avg_sq p_targ | n n_clip | hyper | beta1 beta2 | eps weight_decay clip polyak | stream
    "uavgnn_adamw_polyak": (_I, [_P, _P, _P, _P, _P, _LL, _LL, _P, _D, _D, _F, _F, _F, _F, _P]),
    #                    x_src E F_src x_dst F_dst seg_off dst_order N | W_s b_s W_d b_d attn | nh D slope | out d_out ld_out |
    #                    attn_save dW_s db_s dW_d db_d dattn dW_r db_r workspace | workspace_bytes stream
    "uavgnn_gatv2_bwd": (_I, [_P, _I, _I, _P, _I, _P, _P, _I, _P, _P, _P, _P, _P, _I, _I, _F, _P, _P, _I,
                              _P, _P, _P, _P, _P, _P, _P, _P, _P, _SZ, _P]),
    #                               seen_params near_params nh D slope image stream
    "uavgnn_gatv2_hetero_prepare": (_I, [_PP, _PP, _I, _I, _F, _P, _P]),
    #                        fields n_fields E capacity state stream
    "uavgnn_replay_commit": (_I, [_PLL, _I, _I, _I, _P, _P]),
    #                   int_consts f64_consts B | actions avail_moves pos_ubs pos_gts prior avg_rate t run_f32 n_colls d_u2g d_u2u gt_ubs
    #                   gt_rb rate_per_gt rate_per_ubs mask_collision reward done obs_gt obs_ubs obs_agent state | stream
    "uavgnn_env_step": (_I, [_PI32, _PD, _I, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    #                             state rng capacity B prio beta idx weights status workspace stream
    "uavgnn_replay_prio_sample": (_I, [_P, _P, _I, _I, _P, _D, _P, _P, _P, _P, _P]),
}


@pytest.mark.parametrize("name", sorted(_PINNED))
def test_derived_signature_is_the_hand_written_one(name):
    want_res, want_args = _PINNED[name]
    res, args = _lib.SIGNATURES[name]
    assert res is want_res, (name, res)
    assert len(args) == len(want_args), (name, len(args), len(want_args))
    for i, (a, w) in enumerate(zip(args, want_args)):
        assert a is w, (name, i, a, w)


def test_pinned_long_entries_have_the_length_the_header_gives_them():
    assert len(_PINNED["uavgnn_gatv2_bwd"][1]) == 30 and len(_PINNED["uavgnn_env_step"][1]) == 3 + 22 + 1


_SYNTHETIC = """
/* a header of the test's own */
#ifndef UAVGNN_T_H
#define UAVGNN_T_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif
#define UAVGNN_T_ONE 1 /* a comment behind a value */
#define UAVGNN_T_NEG (-7)
typedef void* uavgnn_stream_t;
int uavgnn_t_void(void);   /* host only */
const char* uavgnn_t_text(int code);
size_t uavgnn_t_mixed(const float* x, /* between parameters */ long long ld, double beta,
                      const int32_t* int_consts,
                      float slope, const float* const* seen_params, uavgnn_stream_t stream);
long long uavgnn_t_bytes(int n);   /* host only */
#ifdef __cplusplus
}
#endif
#endif
"""


def test_parser_on_a_text_of_its_own():
    sigs, consts = _lib.parse_header(_SYNTHETIC)
    assert consts == {"UAVGNN_T_ONE": 1, "UAVGNN_T_NEG": -7}, "the include guard has no value and is no constant"
    assert list(sigs) == ["uavgnn_t_void", "uavgnn_t_text", "uavgnn_t_mixed", "uavgnn_t_bytes"]
    assert sigs["uavgnn_t_void"] == (_I, [])
    assert sigs["uavgnn_t_text"] == (ctypes.c_char_p, [_I])
    assert sigs["uavgnn_t_mixed"] == (_SZ, [_P, _LL, _D, _PI32, _F, _PP, _P])
    assert sigs["uavgnn_t_bytes"] == (_LL, [_I])


@pytest.mark.parametrize("decl", ["int uavgnn_t_bad(const float* x, short n, uavgnn_stream_t stream);",      # an unknown scalar
                                  "short uavgnn_t_bad(int n);",                                               # ... as the result
                                  "int uavgnn_t_bad(int);",                                                   # a parameter without a name
                                  "int uavgnn_t_bad();",                                                      # no prototype in C
                                  "int uavgnn_t_bad(int n); int uavgnn_t_bad(int n);",                        # declared twice
                                  "int some_global;"])                                                        # not an entry point
def test_parser_refuses_what_it_cannot_read_and_quotes_it(decl):
    with pytest.raises(_lib.UavGnnError) as e:
        _lib.parse_header("int uavgnn_t_ok(int n);\n" + decl)
    assert decl.split(";")[0].strip() in str(e.value), "the message quotes the declaration"


def test_missing_header_is_an_error_with_its_path(monkeypatch, tmp_path):
    monkeypatch.setattr(_lib, "HEADER_PATH", str(tmp_path / "include" / "uavgnn.h"))
    with pytest.raises(_lib.UavGnnError, match=re.escape(str(tmp_path / "include" / "uavgnn.h"))):
        _lib._read_header()


def test_constants_are_the_headers():
    build_lib()
    assert _lib.UAVGNN_VERSION == 101 == _lib.lib().uavgnn_version()
    assert _lib.UAVGNN_EINVAL == -1000 and _lib.UAVGNN_EUNSUPPORTED == -1001 and _lib.UAVGNN_EWORKSPACE == -1002
    bits = [_lib.UAVGNN_GEMM_ACCUMULATE, _lib.UAVGNN_GEMM_RELU, _lib.UAVGNN_GEMM_STAGING_INTERLEAVED, _lib.UAVGNN_GEMM_TILE_128,
            _lib.UAVGNN_GEMM_TILE_64]
    assert bits == [1, 2, 4, 8, 16]
    assert (_lib.UAVGNN_TD_NSTEP, _lib.UAVGNN_TD_LAMBDA, _lib.UAVGNN_GRU_STAGING_BLOCKS) == (0, 1, 1)
    assert [_lib.UAVGNN_WS_GATV2_BWD, _lib.UAVGNN_WS_DEGREE_ORDER, _lib.UAVGNN_WS_CSC_TRANSPOSE, _lib.UAVGNN_WS_GRU_PLANES,
            _lib.UAVGNN_WS_GRU_BWD_PLANES, _lib.UAVGNN_WS_GEMM_PLANES, _lib.UAVGNN_WS_GEMM_TN_PARTIALS, _lib.UAVGNN_WS_K1_IMAGE] == list(range(1, 9))
    assert not hasattr(_lib, "UAVGNN_H"), "the include guard is no constant"
