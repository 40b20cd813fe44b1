// SPDX-License-Identifier: Apache-2.0
// pybind11 bindings for the gfx950 HIP kernels.
//
// Deliberately ATen-free: kernels take raw device pointers (data_ptr()),
// sizes and the torch HIP stream handle — the .so links only HIP runtime +
// Python, so it builds with bare hipcc and travels in-tree.

#include <pybind11/pybind11.h>
#include <cstdint>
#include <string>

namespace py = pybind11;
using i64 = int64_t;

void ls_spmv(uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t, i64,
             i64, int, int, bool, uintptr_t, int, bool, int, int, i64);
void ls_spmv_select(i64, i64, int, bool, int, bool, int, int, i64,
                    const char**, int*);
void ls_spmv_affine(uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                    uintptr_t, uintptr_t, i64, int, int, bool, uintptr_t,
                    uintptr_t, uintptr_t, i64, uintptr_t, int, int,
                    uintptr_t);
void ls_affine_const_tiles(uintptr_t, uintptr_t, uintptr_t, uintptr_t, i64,
                           int, int, uintptr_t);
int ls_affine_tile();
int ls_affine_group(int, int);
int ls_affine_const_f32_nd();
void ls_spmm(uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t, i64,
             i64, i64, i64, i64, int, int, bool, int, uintptr_t);
int ls_spmm_narrow_kmax();
void ls_spmv_rows(uintptr_t, i64, uintptr_t, uintptr_t, uintptr_t,
                  uintptr_t, uintptr_t, int, int, bool, uintptr_t);
void ls_cg_fused(uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                 uintptr_t, uintptr_t, i64, int, uintptr_t);
void ls_gs_dots(uintptr_t, i64, int, uintptr_t, uintptr_t, i64, bool, int,
                uintptr_t);
i64 ls_segsort_temp_bytes(i64, i64, uintptr_t, uintptr_t, int, int, int,
                          uintptr_t);
void ls_segsort_pairs(uintptr_t, i64, uintptr_t, uintptr_t, uintptr_t,
                      uintptr_t, i64, i64, uintptr_t, uintptr_t, int, int,
                      int, uintptr_t);
void ls_spmv_affine2(uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                     uintptr_t, i64, i64, i64, int, bool, int, bool,
                     uintptr_t);
void ls_spgemm_row_ub(uintptr_t, uintptr_t, uintptr_t, uintptr_t, i64, int,
                      uintptr_t);
void ls_spgemm_bin_count(uintptr_t, uintptr_t, i64, uintptr_t, uintptr_t);
void ls_spgemm_row_ub_bins(uintptr_t, uintptr_t, uintptr_t, uintptr_t, i64,
                           uintptr_t, int, uintptr_t);
void ls_spgemm_affine(uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                      int, int, uintptr_t, int, uintptr_t, uintptr_t,
                      uintptr_t, uintptr_t, uintptr_t, i64, int, int,
                      uintptr_t);
void ls_spgemm_affine_out(uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                          uintptr_t, uintptr_t, uintptr_t, uintptr_t, int,
                          uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                          uintptr_t, i64, int, int, uintptr_t);
void ls_spgemm_compact_rows(uintptr_t, i64, uintptr_t, uintptr_t,
                            uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                            int, int, uintptr_t);
void ls_spgemm_bin_scatter(uintptr_t, uintptr_t, i64, uintptr_t,
                           uintptr_t, uintptr_t);
void ls_spgemm_merge_symbolic(int, uintptr_t, i64, uintptr_t, uintptr_t,
                              uintptr_t, uintptr_t, uintptr_t, int,
                              uintptr_t);
void ls_spgemm_merge_numeric(int, uintptr_t, i64, uintptr_t, uintptr_t,
                             uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                             uintptr_t, uintptr_t, uintptr_t, int, int,
                             uintptr_t, uintptr_t);
void ls_spgemm_symbolic_lds(int, uintptr_t, i64, uintptr_t, uintptr_t,
                            uintptr_t, uintptr_t, uintptr_t, int,
                            uintptr_t);
void ls_spgemm_numeric_lds(int, uintptr_t, i64, uintptr_t, uintptr_t,
                           uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                           uintptr_t, uintptr_t, uintptr_t, int, int,
                           uintptr_t, int, uintptr_t);
void ls_spgemm_symbolic_global(uintptr_t, uintptr_t, uintptr_t, i64,
                               uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                               uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                               int, int, uintptr_t, uintptr_t, uintptr_t,
                               uintptr_t);
void ls_spgemm_numeric_global_fill(uintptr_t, uintptr_t, uintptr_t, i64,
                                   uintptr_t, uintptr_t, uintptr_t,
                                   uintptr_t, uintptr_t, uintptr_t,
                                   uintptr_t, uintptr_t, uintptr_t,
                                   uintptr_t, int, int, int, uintptr_t,
                                   uintptr_t, uintptr_t, uintptr_t);
void ls_spgemm_global_compact(uintptr_t, i64, uintptr_t, uintptr_t,
                              uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                              uintptr_t, uintptr_t, int, int, uintptr_t);
void ls_spgemm_global_compact_sorted(uintptr_t, i64, uintptr_t, uintptr_t,
                                     uintptr_t, uintptr_t, uintptr_t,
                                     uintptr_t, uintptr_t, uintptr_t, int,
                                     int, uintptr_t);
void ls_csr_to_dense(uintptr_t, uintptr_t, uintptr_t, uintptr_t, i64, i64,
                     int, int, uintptr_t);
void ls_dense_to_csr_nnz(uintptr_t, uintptr_t, i64, i64, int, uintptr_t);
void ls_dense_to_csr_fill(uintptr_t, uintptr_t, uintptr_t, uintptr_t, i64,
                          i64, int, int, uintptr_t);
void ls_diagonal(uintptr_t, uintptr_t, uintptr_t, uintptr_t, i64, i64, int,
                 int, uintptr_t);
void ls_axpby(uintptr_t, uintptr_t, uintptr_t, uintptr_t, i64, bool, bool,
              int, uintptr_t);
void ls_vdot(uintptr_t, uintptr_t, uintptr_t, i64, bool, int, uintptr_t);
void ls_jacobi(uintptr_t, uintptr_t, uintptr_t, uintptr_t, double, i64,
               int, uintptr_t);
void ls_bicgstab_p(uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                   uintptr_t, uintptr_t, i64, int, uintptr_t);
void ls_bicgstab_s(uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                   i64, int, uintptr_t);
void ls_vdot2(uintptr_t, uintptr_t, uintptr_t, i64, int, uintptr_t);
void ls_bicgstab_xr(uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                    uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                    uintptr_t, uintptr_t, i64, int, uintptr_t);
int ls_bicgstab_grid_cap();
int ls_bicgstab_per_block();
void ls_block_gram(uintptr_t, i64, int, uintptr_t, i64, int, uintptr_t,
                   uintptr_t, i64, i64, bool, int, uintptr_t);
void ls_block_update(uintptr_t, i64, int, int, uintptr_t, i64, int,
                     uintptr_t, uintptr_t, i64, int, uintptr_t, uintptr_t,
                     i64, int, uintptr_t, bool, i64, int, uintptr_t);
void ls_block_residual(uintptr_t, i64, uintptr_t, i64, uintptr_t, i64,
                       uintptr_t, uintptr_t, uintptr_t, i64, int, i64, int,
                       uintptr_t);
int ls_block_kmax();
int ls_block_gram_grid_cap();
int ls_block_gram_per_block();
int ls_block_update_grid_cap();
int ls_block_update_per_block();
int ls_block_residual_grid_cap();
int ls_block_residual_per_block();
void ls_sptrsv(uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t,
               uintptr_t, uintptr_t, i64, int, i64, i64, uintptr_t, i64,
               uintptr_t, i64, bool, bool, int, int, int, uintptr_t);
void ls_ilu0_factor(uintptr_t, uintptr_t, uintptr_t, uintptr_t, uintptr_t,
                    uintptr_t, uintptr_t, i64, i64, uintptr_t, i64, uintptr_t,
                    i64, bool, int, int, int, uintptr_t);
int ls_sptrsv_kmax();
int ls_sptrsv_chain_rows();
int ls_sptrsv_grid_cap();
void ls_fsai_rows(uintptr_t, uintptr_t, i64, uintptr_t, uintptr_t, uintptr_t,
                  i64, i64, i64, i64, i64, uintptr_t, uintptr_t, int, int,
                  int, int, uintptr_t);
int ls_fsai_max_row();
int ls_fsai_narrow();
int ls_fsai_grid_cap();

PYBIND11_MODULE(_hip_kernels, m) {
  m.doc() = "legate_sparse gfx950 HIP kernels";
  m.def("spmv", &ls_spmv);
  // (kernel, W) that spmv runs for these arguments: "vector", "vector_nt",
  // "vector_swz", "pair", "pair_swz", "pair2" with the sub-wave width,
  // "sten" with NP, "pairu" with its W, "stream" with PE
  m.def("spmv_select",
        [](i64 n_rows, i64 nnz, int dtype, bool accumulate, int w_override,
           bool nt, int pair, int swz, i64 max_nnz) {
          const char* name = nullptr;
          int W = 0;
          ls_spmv_select(n_rows, nnz, dtype, accumulate, w_override, nt,
                         pair, swz, max_nnz, &name, &W);
          return py::make_tuple(std::string(name), W);
        },
        py::arg("n_rows"), py::arg("nnz"), py::arg("dtype"),
        py::arg("accumulate"), py::arg("w_override"), py::arg("nt"),
        py::arg("pair"), py::arg("swz"), py::arg("max_nnz"));
  m.def("spmv_affine", &ls_spmv_affine);
  m.def("affine_const_tiles", &ls_affine_const_tiles);
  m.attr("AFFINE_TILE") = ls_affine_tile();
  m.def("affine_group", &ls_affine_group);
  m.attr("AFFINE_CONST_F32_ND") = ls_affine_const_f32_nd();
  m.def("spmv_rows", &ls_spmv_rows);
  m.def("spmm", &ls_spmm);
  m.attr("SPMM_NARROW_KMAX") = ls_spmm_narrow_kmax();
  m.def("cg_fused", &ls_cg_fused);
  m.def("gs_dots", &ls_gs_dots);
  m.def("segsort_temp_bytes", &ls_segsort_temp_bytes);
  m.def("segsort_pairs", &ls_segsort_pairs);
  m.def("spmv_affine2", &ls_spmv_affine2);
  m.def("spgemm_row_ub", &ls_spgemm_row_ub);
  m.def("spgemm_bin_count", &ls_spgemm_bin_count);
  m.def("spgemm_row_ub_bins", &ls_spgemm_row_ub_bins);
  m.def("spgemm_affine", &ls_spgemm_affine);
  m.def("spgemm_affine_out", &ls_spgemm_affine_out);
  m.def("spgemm_compact_rows", &ls_spgemm_compact_rows);
  m.def("spgemm_bin_scatter", &ls_spgemm_bin_scatter);
  m.def("spgemm_merge_symbolic", &ls_spgemm_merge_symbolic);
  m.def("spgemm_merge_numeric", &ls_spgemm_merge_numeric);
  m.def("spgemm_symbolic_lds", &ls_spgemm_symbolic_lds);
  m.def("spgemm_numeric_lds", &ls_spgemm_numeric_lds);
  m.def("spgemm_symbolic_global", &ls_spgemm_symbolic_global);
  m.def("spgemm_numeric_global_fill", &ls_spgemm_numeric_global_fill);
  m.def("spgemm_global_compact", &ls_spgemm_global_compact);
  m.def("spgemm_global_compact_sorted", &ls_spgemm_global_compact_sorted);
  m.attr("spgemm_global_chunk") = 2048;
  m.def("csr_to_dense", &ls_csr_to_dense);
  m.def("dense_to_csr_nnz", &ls_dense_to_csr_nnz);
  m.def("dense_to_csr_fill", &ls_dense_to_csr_fill);
  m.def("diagonal", &ls_diagonal);
  m.def("axpby", &ls_axpby);
  m.def("vdot", &ls_vdot);
  m.def("jacobi", &ls_jacobi);
  m.def("bicgstab_p", &ls_bicgstab_p);
  m.def("bicgstab_s", &ls_bicgstab_s);
  m.def("vdot2", &ls_vdot2);
  m.def("bicgstab_xr", &ls_bicgstab_xr);
  // the four BiCGSTAB kernels share one launch shape; exported per kernel
  // so a test can size an input past cap * per_block
  for (const char* k : {"BICGSTAB_P", "BICGSTAB_S", "VDOT2", "BICGSTAB_XR"}) {
    m.attr((std::string(k) + "_GRID_CAP").c_str()) = ls_bicgstab_grid_cap();
    m.attr((std::string(k) + "_PER_BLOCK").c_str()) = ls_bicgstab_per_block();
  }
  // LOBPCG block kernels (block_ops.hip); PER_BLOCK counts rows
  m.def("block_gram", &ls_block_gram);
  m.def("block_update", &ls_block_update);
  m.def("block_residual", &ls_block_residual);
  m.attr("BLOCK_KMAX") = ls_block_kmax();
  m.attr("BLOCK_GRAM_GRID_CAP") = ls_block_gram_grid_cap();
  m.attr("BLOCK_GRAM_PER_BLOCK") = ls_block_gram_per_block();
  m.attr("BLOCK_UPDATE_GRID_CAP") = ls_block_update_grid_cap();
  m.attr("BLOCK_UPDATE_PER_BLOCK") = ls_block_update_per_block();
  m.attr("BLOCK_RESIDUAL_GRID_CAP") = ls_block_residual_grid_cap();
  m.attr("BLOCK_RESIDUAL_PER_BLOCK") = ls_block_residual_per_block();
  // level-scheduled triangular solve and ILU(0) (sptrsv.hip)
  m.def("sptrsv", &ls_sptrsv);
  m.def("ilu0_factor", &ls_ilu0_factor);
  m.attr("SPTRSV_KMAX") = ls_sptrsv_kmax();
  m.attr("SPTRSV_CHAIN_ROWS") = ls_sptrsv_chain_rows();
  m.attr("SPTRSV_GRID_CAP") = ls_sptrsv_grid_cap();
  // FSAI setup (fsai.hip)
  m.def("fsai_rows", &ls_fsai_rows);
  m.attr("FSAI_MAX_ROW") = ls_fsai_max_row();
  m.attr("FSAI_NARROW") = ls_fsai_narrow();
  m.attr("FSAI_GRID_CAP") = ls_fsai_grid_cap();
  m.attr("arch") = "gfx950";
  m.attr("spgemm_lds_bins") = py::make_tuple(48, 128, 1024, 4096);
}
