"""Every entry point include/peekvit_hip.h declares has a test that calls it DIRECTLY (through its peekvit_amd.ops wrapper or the ctypes
binding), named below.  A new entry point cannot land without one: the ledger's keys must be exactly the declared set, and every named
test must exist (found with ast, nothing imported).  Model-level tests that reach a kernel only inside a forward do not count."""
import ast
import os
import re

from conftest import REPO

LEDGER = {
    # queries and host-side functions
    "pv_version": ["test_host_contract.py::test_library_exports_every_declared_symbol"],
    "pv_arch": ["test_host_contract.py::test_library_exports_every_declared_symbol"],
    "pv_operand_type": ["test_host_contract.py::test_library_exports_every_declared_symbol"],
    "pv_error_string": ["test_host_contract.py::test_library_exports_every_declared_symbol"],
    "pv_workspace_size": ["test_host_contract.py::test_workspace_size_matches_the_documented_formulas"],
    "pv_gemm_args_size": ["test_host_contract.py::test_library_refuses_a_struct_of_another_length"],
    "pv_gemm_tile_rows": ["test_host_contract.py::test_library_refuses_a_struct_of_another_length",
                          "test_hip_ops.py::test_gemm_gelu_is_elementwise_exact_on_both_tile_kernels",
                          "test_hip_gemm_exact.py::test_gemm128_every_epilogue_exact", "test_hip_gemm_exact.py::test_gemm256_plain_epilogues_exact",
                          "test_gemm_exact_host.py::test_dispatcher_keeps_256_row_kernels_inside_their_stride_limits"],
    # patch gather and token prologue
    "pv_cast_f32_bf16": ["test_hip_ops.py::test_cast_and_im2col_bit_exact"],
    "pv_im2col_bf16": ["test_hip_ops.py::test_cast_and_im2col_bit_exact", "test_hip_entry_points.py::test_im2col_u8_equals_im2col_of_normalised_image"],
    "pv_patch_embed_f32": ["test_hip_ops.py::test_patch_embed_without_a_patch_matrix_is_bit_identical_to_im2col_plus_gemm"],
    "pv_im2col_u8_bf16": ["test_hip_entry_points.py::test_im2col_u8_equals_im2col_of_normalised_image"],
    "pv_token_prologue": ["test_hip_entry_points.py::test_token_prologue"],
    # LayerNorm and GEMMs
    "pv_layernorm_bf16": ["test_hip_ops.py::test_layernorm", "test_hip_entry_points.py::test_layernorm_every_bucket",
                          "test_hip_entry_points.py::test_layernorm_two_pass_variance", "test_hip_entry_points.py::test_layernorm_strided_input"],
    "pv_rowstat_finalize": ["test_hip_ops.py::test_layernorm_folded_into_gemms"],
    "pv_gemm_bf16": ["test_hip_ops.py::test_gemm_epilogues", "test_hip_gemm_exact.py::test_gemm128_every_epilogue_exact",
                     "test_hip_gemm_exact.py::test_gemm256_features_exact", "test_hip_gemm_exact.py::test_gemm256_plain_epilogues_exact",
                     "test_hip_gemm_exact.py::test_gemm256_persistent_launch_exact", "test_hip_gemm_exact.py::test_gemm256_split_k_exact",
                     "test_hip_gemm_exact.py::test_gemm_fused_layernorm_fp32_output_exact"],
    "pv_gemm_tn_bf16": ["test_hip_backward.py::test_gemm_tn_weight_gradient", "test_hip_gemm_exact.py::test_gemm_tn_exact"],
    # attention
    "pv_attention_bf16": ["test_hip_ops.py::test_attention", "test_hip_attention_forward_rows.py::test_resident_forward_rows_every_instantiation",
                          "test_hip_attention_forward_rows.py::test_resident_forward_maps_workgroups_to_images_and_heads", "test_hip_attention_forward_rows.py::test_streaming_forward_rows_every_instantiation"],
    "pv_attention_rows_bf16": ["test_hip_ops.py::test_attention_rows", "test_hip_attention_forward_rows.py::test_class_row_forward_rows",
                               "test_hip_attention_forward_rows.py::test_class_row_forward_on_peaked_rows"],
    "pv_attention_rows_bwd_bf16": ["test_hip_backward.py::test_attention_rows_backward"],
    "pv_attention_bwd_bf16": ["test_hip_backward.py::test_attention_backward"],
    "pv_attention_lse_bf16": ["test_hip_backward.py::test_attention_backward_from_the_forward_statistics",
                              "test_hip_attention_forward_rows.py::test_resident_forward_rows_every_instantiation", "test_hip_attention_forward_rows.py::test_resident_forward_of_a_single_token",
                              "test_hip_attention_forward_rows.py::test_resident_forward_with_statistics_refuses_a_length_past_its_range"],
    "pv_attention_bwd_lse_bf16": ["test_hip_backward.py::test_persistent_attention_backward_every_instantiation"],
    # precision mode bf16x3
    "pv_split3_f32_bf16": ["test_hip_precision.py::test_split3_layout_and_accuracy"],
    "pv_im2col_split_bf16": ["test_hip_entry_points.py::test_im2col_split_planes"],
    "pv_layernorm_split_bf16": ["test_hip_entry_points.py::test_layernorm_every_bucket", "test_hip_entry_points.py::test_layernorm_strided_input"],
    "pv_attention_f32_split": ["test_hip_precision.py::test_attention_f32", "test_hip_attention_forward_rows.py::test_fp32_forward_rows_every_tile_count",
                               "test_hip_attention_forward_rows.py::test_fp32_input_forwards_refuse_one_tile_count_past_their_range"],
    "pv_attention_split_bf16": ["test_hip_ops.py::test_attention_split_scores", "test_hip_attention_forward_rows.py::test_split_score_forward_rows_every_tile_count",
                                "test_hip_attention_forward_rows.py::test_fp32_input_forwards_refuse_one_tile_count_past_their_range"],
    # split-K finishes and backward building blocks
    "pv_sum_slices_f32": ["test_hip_backward.py::test_sum_slices", "test_hip_gemm_exact.py::test_gemm_tn_exact"],
    "pv_sum_slices_add_f32": ["test_hip_entry_points.py::test_sum_slices_add"],
    "pv_sum_slices_act_bf16": ["test_hip_entry_points.py::test_sum_slices_act", "test_hip_entry_points.py::test_sum_slices_act_range_flag"],
    "pv_sum_slices_add_ln_f32": ["test_hip_entry_points.py::test_sum_slices_add_ln"],
    "pv_transpose_bf16": ["test_hip_backward.py::test_transpose_exact"],
    "pv_layernorm_bwd": ["test_hip_backward.py::test_layernorm_backward"],
    "pv_layernorm_bwd16": ["test_hip_backward.py::test_layernorm_backward_with_a_16_bit_residual_gradient"],
    "pv_layernorm_bwd_masked": ["test_hip_backward.py::test_layernorm_backward_masked"],
    "pv_masked_residual": ["test_hip_entry_points.py::test_masked_residual"],
    "pv_gelu_bf16": ["test_hip_backward.py::test_gelu_forward_backward"],
    "pv_gelu_bwd_bf16": ["test_hip_backward.py::test_gelu_forward_backward"],
    "pv_colsum_f32": ["test_hip_backward.py::test_colsum"],
    "pv_scatter_tokens": ["test_hip_backward.py::test_scatter_tokens", "test_hip_token_selection.py::test_gather_scatter_tokens_are_pure_copies"],
    # pooling, head, ranking, compaction, residual gate
    "pv_cls_pool": ["test_hip_ops.py::test_cls_pool_and_head", "test_hip_entry_points.py::test_cls_pool"],
    "pv_head_f32": ["test_hip_ops.py::test_cls_pool_and_head", "test_hip_entry_points.py::test_head_both_kernels"],
    "pv_token_norm": ["test_hip_ops.py::test_rank_path_bit_exact_vs_reference_golden",
                      "test_hip_token_selection.py::test_token_norm_per_element_against_fp64",
                      "test_hip_token_selection.py::test_token_norm_of_class_rows_only_writes_nothing"],
    "pv_rank_topk": ["test_hip_entry_points.py::test_rank_topk_without_gap", "test_hip_token_selection.py::test_rank_topk_exact_against_stable_sort"],
    "pv_rank_topk_partials": ["test_hip_entry_points.py::test_rank_topk_without_gap",
                              "test_hip_token_selection.py::test_rank_topk_partials_exact_on_integer_sums"],
    "pv_rank_topk_gap": ["test_hip_ops.py::test_rank_ties_lowest_index_first_and_edges",
                         "test_hip_models.py::test_rank_topk_reports_the_gap_at_the_keep_boundary",
                         "test_hip_token_selection.py::test_rank_topk_exact_against_stable_sort"],
    "pv_rank_topk_partials_gap": ["test_hip_models.py::test_rank_topk_reports_the_gap_at_the_keep_boundary",
                                  "test_hip_token_selection.py::test_rank_topk_partials_exact_on_integer_sums"],
    "pv_gather_tokens": ["test_hip_ops.py::test_rank_ties_lowest_index_first_and_edges",
                         "test_hip_token_selection.py::test_gather_scatter_tokens_are_pure_copies"],
    "pv_residual_gate": ["test_hip_ops.py::test_residual_gate"],
    "pv_residual_gate_bwd": ["test_hip_backward.py::test_residual_gate_backward"],
    # A-ViT packed halting
    "pv_attention_varlen_bf16": ["test_hip_avit.py::test_varlen_attention_against_fp64", "test_hip_avit.py::test_varlen_attention_every_tile_bound"],
    "pv_act_step": ["test_hip_avit.py::test_act_step_against_torch_restatement", "test_hip_avit.py::test_act_step_production_sizes"],
}
# entry points whose op-level test drives them through a torch.autograd.Function of peekvit_amd/train_engine.py (that class's backward IS
# the launch): entry -> the class
AUTOGRAD = {"pv_residual_gate_bwd": "GateFn"}


def declared_entry_points():
    """Names of the functions include/peekvit_hip.h declares (comments stripped; pv_gemm_args is a struct)."""
    src = open(os.path.join(REPO, "include", "peekvit_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    return set(re.findall(r"^\s*(?:const\s+)?\w+\s*\*?\s*(pv_\w+)\s*\(", src, flags=re.M))


def _test_functions(path):
    """Top-level test function names of a test module, by ast (the module is not imported)."""
    tree = ast.parse(open(path).read(), filename=path)
    return {n.name for n in tree.body if isinstance(n, (ast.FunctionDef, ast.AsyncFunctionDef)) and n.name.startswith("test_")}


def test_ledger_keys_are_exactly_the_declared_entry_points():
    declared = declared_entry_points()
    assert len(declared) >= 52
    assert set(LEDGER) == declared, f"missing: {sorted(declared - set(LEDGER))}, not declared: {sorted(set(LEDGER) - declared)}"


def test_every_ledger_test_exists_and_calls_its_entry_point():
    ops_src = open(os.path.join(REPO, "peekvit_amd", "ops.py")).read()
    eng_src = open(os.path.join(REPO, "peekvit_amd", "train_engine.py")).read()
    tests_dir = os.path.join(REPO, "tests")
    found = {}
    for entry, ids in LEDGER.items():
        assert ids, f"{entry}: no direct test named"
        for tid in ids:
            fname, _, name = tid.partition("::")
            path = os.path.join(tests_dir, fname)
            assert os.path.isfile(path), f"{entry}: {fname} does not exist"
            if path not in found:
                found[path] = _test_functions(path)
            assert name in found[path], f"{entry}: {tid} does not exist"
    # and the entry point is reachable by name from that test: the symbol itself, or an ops wrapper whose body calls it
    wrappers = {}
    for node in ast.parse(ops_src).body:
        if isinstance(node, ast.FunctionDef):
            for sym in re.findall(r"\b(pv_\w+)\(", ast.get_source_segment(ops_src, node)):
                wrappers.setdefault(sym, set()).add(node.name)
    for entry, ids in LEDGER.items():
        for tid in ids:
            fname, _, name = tid.partition("::")
            path = os.path.join(tests_dir, fname)
            src = open(path).read()
            fn = next(n for n in ast.parse(src).body if isinstance(n, ast.FunctionDef) and n.name == name)
            body = ast.get_source_segment(src, fn)
            direct = re.search(rf"\b{entry}\b", body) is not None
            via = any(re.search(rf"\bops\.{w}\(", body) for w in wrappers.get(entry, ()))
            if entry in AUTOGRAD:
                cls = next(n for n in ast.parse(eng_src).body if isinstance(n, ast.ClassDef) and n.name == AUTOGRAD[entry])
                calls = ast.get_source_segment(eng_src, cls)
                via = re.search(rf"\b{AUTOGRAD[entry]}\.apply\(", body) is not None and any(re.search(rf"\bops\.{w}\(", calls) for w in wrappers[entry])
            assert direct or via, f"{tid} does not call {entry} (nor an ops wrapper that does)"
