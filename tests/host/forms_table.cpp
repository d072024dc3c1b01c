// The planning rules of gdrf_amd/csrc/forms.h as a table, without a GPU.  Build: c++ -std=c++17 -o forms_table tests/host/forms_table.cpp
//   forms_table          reads one shape per line from stdin:
//                          n n_cap M K V D esz ssz split stored_t rows_form csr hyper_tn learn_z ard per kind predict_mode unwhitened
//                        and prints, per shape, the 17 slots of gdrf_last_forms of a fresh context after one step on n rows and one
//                        gdrf_predict(predict_mode) on n rows (0: the stage did not run, or its shape does not fit), then the split counts
//                        ns, nst, ns1 of A_k, ns of G^T and ns of the hyper-TN form
//   forms_table max      prints the highest code of each named slot
//   forms_table mm       reads "Mp esz ssz batch beside_chain" per line (a product of esz-byte elements in a context whose solve type has
//                        ssz bytes) and prints mm_plan's form, slices and reduction indices per slice
#include "../../gdrf_amd/csrc/forms.h"

#include <cstdio>
#include <cstring>

using namespace gdrf::forms;

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "max")) {
    std::printf("wbar %d\na_k %d\nfwd_t %d\nloc %d\nrows %d\ngt %d\nhyper %d\npredict %d\nmm_chain %d\nmm_sbar %d\n", WBAR_LAST, AK_LAST, FWD_T_LAST, LOC_LAST,
                ROWS_LAST, GT_LAST, HYPER_LAST, PREDICT_LAST, MM_LAST, MM_LAST);
    return 0;
  }
  if (argc > 1 && !std::strcmp(argv[1], "mm")) {
    int Mp, esz, ssz, batch, beside;
    while (std::scanf("%d %d %d %d %d", &Mp, &esz, &ssz, &batch, &beside) == 5) {
      const MmPlan m = mm_plan(Mp, esz, batch, mm_tiles(Mp, esz), mm_slab_bytes(Mp, ssz), beside != 0);
      std::printf("%d %d %d\n", m.form, m.S, m.kw);
    }
    return 0;
  }
  long long n, n_cap;
  int M, K, V, D, esz, ssz, split, stored_t, rows_form, csr, hyper_tn, learn_z, ard, per, kind, mode, unwhitened;
  while (std::scanf("%lld %lld %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d", &n, &n_cap, &M, &K, &V, &D, &esz, &ssz, &split, &stored_t, &rows_form, &csr,
                    &hyper_tn, &learn_z, &ard, &per, &kind, &mode, &unwhitened) == 19) {
    FormShape f;
    f.n = n; f.n_cap = n_cap; f.M = M; f.Mp = (int)round_up(M, F_MPAD); f.K = K; f.V = V; f.D = D; f.esz = esz; f.ssz = ssz; f.split = split;
    f.stored_t = stored_t != 0; f.rows_form = rows_form; f.csr = csr != 0;
    f.hyper_tn = hyper_tn; f.learn_z = learn_z; f.ard = ard; f.per = per; f.kind = kind;
    f.nsplit_cap = nsplit_cap_rule(K, f.Mp, n_cap, esz); f.predict_mode = mode; f.unwhitened = unwhitened != 0;
    const WbarPlan w = wbar_plan(f);
    const AkPlan a = ak_plan(f);
    const FwdTPlan t = fwd_t_plan(f);
    const LocPlan l = loc_plan(f);
    const UbarPlan u = ubar_plan(f);
    const RowsPlan r = rows_plan(f);
    const GtPlan g = gt_plan(f);
    const HyperPlan h = hyper_plan(f);
    const PredictPlan p = predict_plan(f);
    std::printf("%d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d %d  %d %d %d %d %d\n", w.fits ? w.form : 0, w.fits ? w.nslice : 0, a.form, a.kgroups, t.form, t.KG,
                l.form, u.kq, r.fits ? r.form : 0, r.fits ? r.nkt : 0, r.fits ? r.nvt : 0, g.form, h.form, p.fits ? p.form : 0, p.fits ? p.NB : 0, mm_chain_plan(f).form, mm_sbar_plan(f).form, a.ns, a.nst,
                a.ns1, g.ns, h.ns);
  }
  return 0;
}
