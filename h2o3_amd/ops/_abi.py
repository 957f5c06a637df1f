"""C signatures of every exported `h2o_*` function of the HIP libraries
(ops/csrc/<library>.hip), applied by `_native.get_lib` when it loads a library.

One line per function: name, return kind, argument kinds in order, in the
letters of the `struct` module:

    P  pointer (device or host; `hipStream_t` too)      i  int
    q  long long        Q  unsigned long long           f  float
    d  double           v  void (return only)

tests/test_native_abi.py compares this table with the prototypes in the
sources, so a kernel wrapper that gains an argument is updated here and
nowhere else.  The host C++ libraries (native/*.cpp) are typed by their
callers.
"""
import ctypes

_TABLE = {
    "dl": """
        h2o_dl_seed_advance  i  PP
        h2o_dl_fwd           i  PPPiiifQPifP
        h2o_dl_bwd           i  PPPPPiiifQPP
        h2o_dl_update        i  PPPPPPPPPiifffffffiiiffP
        h2o_dl_softmax       i  PPPPPPPiifiP
        h2o_dl_mlp_step      i  iPPPPPPPPPPPPPPPiPPPPiifQPiP
        h2o_dl_gemm_ws       q  iii
        h2o_dl_gemm          i  iiiPqqPqqPPqP
    """,
    "dl_shap": """
        h2o_dl_shap_chunk  i
        h2o_dl_shap_pairs  i  iPPPPPPPPPPiiPPqqqiiP
    """,
    "fairness": """
        h2o_fairness_lds_groups  i
        h2o_group_sketch         i  PiPPqiiidiPPPiP
    """,
    "frame": """
        h2o_rollup_multi    i  PiqiPiPP
        h2o_expand_numeric  i  PiqPPPPiiiP
    """,
    "gram": """
        h2o_gram                 i  PPqiPiiiPP
        h2o_glm_irls_chunk       i  i
        h2o_glm_irls             i  PqiiPiiiPfPPPiiffPPiiPPPiiiP
        h2o_gram_split           i  PiiiPPqPP
        h2o_glm_wide_split_grid  i  i
        h2o_glm_wide_split       i  PiiiqPfPPPiiffPPiPPP
        h2o_glm_wide_gram        i  PiiqPiiPiP
        h2o_glm_wide_gram256     i  PiiqPiiPiiP
        h2o_gram_f64             i  PiiqPPiiqPP
        h2o_xv_f64               i  PiiqPdPP
        h2o_xtr_f64              i  PiiqPiqPP
    """,
    "kmeans": """
        h2o_kmeans_assign_resident_per_cu  i  ii
        h2o_kmeans_assign                  i  PqiPPiPPiP
        h2o_xv_resident_per_cu             i  ii
        h2o_xv                             i  PqiPiPiP
        h2o_kmeans_max_k                   i  ii
        h2o_kmeans_part_stride             q  ii
        h2o_kmeans_set_debug               v  i
        h2o_kmeans_resident_per_cu         i  iiif
        h2o_kmeans_lloyd                   i  PPqiPPiPPPPiifP
        h2o_kmeans_sums_resident_per_cu    i  ii
        h2o_kmeans_sums                    i  PPqiiPPPPifP
        h2o_kmeans_reduce                  i  PiqPP
    """,
    "metrics": """
        h2o_logit_hist    i  PPPqiPPP
        h2o_group_reduce  i  PPqiiiPP
    """,
    "tree_eif": """
        h2o_eif_lengths  i  PqiPPPPiiPPiiP
    """,
    "tree_hist": """
        h2o_hist_quad           i  PiPPPPiiiiffPiiiPiqiiPPP
        h2o_hist_bm_set_debug   v  i
        h2o_hist_bm             i  PiPPPPiiiiffPiiPiqiiiPPPP
        h2o_iota_i32            i  PqP
        h2o_hist_build          i  PiiPPPPiiiiffPiiiPiPP
        h2o_hist_build_pk       i  PiiPPPPiiiifqPiiPiPP
        h2o_part_flags          i  PiqqPPPiPPiPPPP
        h2o_hist_sibling        i  PPPiiiiiiiPPPPPP
        h2o_child_work          i  PPPiiiiiiiiPPPP
        h2o_part_offsets        i  PPiiPPPPiiP
        h2o_part_compact        i  PPPiPPPPPPPP
        h2o_part_count          i  PiqqPPiPPiPP
        h2o_part_scatter        i  PiqqPPiPPiPPPPPPPP
        h2o_fill_nid            i  PPiPP
        h2o_leaf_pass           i  PPPPiiPPP
        h2o_seg_sum2            i  PPPPiPP
        h2o_leaf_pos            i  PPiiPPP
        h2o_col_sample          i  iiPiQPP
        h2o_leaf_scatter        i  PPiPPP
        h2o_leaf_update         i  PPiPPP
        h2o_pair_hist4          i  PiqPPPPiPiiiffPPPP
        h2o_pair_hist           i  PiqPPPPiPiiiffPPP
        h2o_gbm_grad            i  PPPiqPPP
        h2o_part_items          i  PiiiPPPP
        h2o_dt_items2           i  iPiiiiiPPPPP
        h2o_dt_items            i  iPiiiiiPPPP
        h2o_dt_offsets          i  PPPPiPPPP
        h2o_dt_sibling          i  PPPiiiiiiPPPPP
        h2o_dt_leaf_vals        i  PPiiPdPP
        h2o_dt_root             i  PqP
        h2o_dt_root_leaf_iota   i  PPqP
        h2o_leaf_scatter_dev    i  PPiPPPP
        h2o_leaf_flag_sums_dev  i  PPPiPPiiPPP
        h2o_leaf_gather_lds     i  ii
        h2o_leaf_gather_items   i  qi
        h2o_leaf_gather_dev     i  PiiiPPPPqiiPPPPPP
        h2o_dt_colmask          i  iPPPPPiiPP
    """,
    "tree_pd": """
        h2o_pd_block_threads  i  ii
        h2o_pd_lds_bytes      q  iii
        h2o_forest_pd_chunk   i  PqiPiPPPPPPiiPiPiiiiPiPqiP
    """,
    "tree_predict": """
        h2o_forest_predict  i  PqPPPPPPPiiPPP
    """,
    "tree_shap": """
        h2o_shap_masks           i  PqiPPPPPPPPPPPiiiPPdP
        h2o_shap_lds_bytes       q  i
        h2o_shap_pairs           i  PiPiPPPPiiiPPdPqiiiiP
        h2o_shap_path_lds_bytes  q  i
        h2o_shap_path            i  PiPPPPPiiiPdPqiP
    """,
    "tree_split": """
        h2o_split_find_b   i  PiiiPPPdddddiPPiP
        h2o_split_find     i  PiiiPPPdddddiPP
        h2o_split_select   i  PPiiiiPPP
        h2o_split_select2  i  PPiiiidiPPPP
        h2o_cat_pairs      i  PiiiiPPPPPdddddiPP
        h2o_cat_pairs2     i  PiiiiPPPPPdddddiPPiPP
        h2o_pair_select    i  PiiiPPPidiPPPPP
        h2o_ua_range       i  PiiiPPP
        h2o_ua_fold        i  PiiiiPPiPPP
    """,
}

_KINDS = {"P": ctypes.c_void_p, "i": ctypes.c_int, "q": ctypes.c_longlong, "Q": ctypes.c_ulonglong,
          "f": ctypes.c_float, "d": ctypes.c_double, "v": None}


def signatures():
    """{library: {function: (return kind, argument kinds)}}."""
    out = {}
    for lib, text in _TABLE.items():
        out[lib] = {}
        for name, ret, *args in map(str.split, text.strip().split("\n")):
            out[lib][name] = (ret, "".join(args))
    return out


def apply(name, lib):
    """Set argtypes / restype of every function the table lists for library
    `name`; a listed symbol the library does not export is an error."""
    for fn, (ret, args) in signatures().get(name, {}).items():
        try:
            f = getattr(lib, fn)
        except AttributeError:
            raise RuntimeError(f"lib{name}.so does not export {fn} (ops/_abi.py lists it)") from None
        f.argtypes = [_KINDS[a] for a in args]
        f.restype = _KINDS[ret]
