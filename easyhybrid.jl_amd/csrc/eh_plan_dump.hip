// eh_plan_dump FILE: prints what eh_plan_model (eh_plan.hpp) makes of descriptors, one JSON line each -- no HIP call, runs without a device.
// FILE holds records of [int32 seq_several_targets | eh_model_desc], the bytes a host binding hands to eh_create / eh_create_seq_targets.
// A refusal prints {"rc", "msg"}; a plan its family, the EhNet in the text of `#define EH_SPEC_NET` (eh_jit.hip), the leaf table of flat
// theta and the state of the normalisation layers.  tests/test_plan.py reads the lines.
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "eh_plan.hpp"

static std::string json_str(const std::string& s) {
    std::string o = "\"";
    for (const char c : s) {
        if (c == '"' || c == '\\') { o += '\\'; o += c; }
        else if ((unsigned char)c < 0x20) { char b[8]; snprintf(b, sizeof b, "\\u%04x", c); o += b; }
        else o += c;
    }
    return o + "\"";
}

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: eh_plan_dump FILE\n"); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    static const char* const family[] = {"none", "seq", "norm", "fused"};
    struct Rec { int32_t several; eh_model_desc d; } rec;
    EhPlan p;
    std::string msg;
    while (fread(&rec, sizeof rec, 1, f) == 1) {
        if (const int rc = eh_plan_model(&rec.d, rec.several != 0, &p, &msg)) { printf("{\"rc\": %d, \"msg\": %s}\n", rc, json_str(msg).c_str()); continue; }
        const EhNet& n = p.net;
        printf("{\"rc\": 0, \"family\": \"%s\", \"act\": %d, \"nbi\": %d, \"nbh\": %d, \"n_theta\": %d, \"g_off\": %d, \"n_acc\": %d, \"n_weights\": %d, ", family[p.family], p.act, p.nbi,
               p.nbh, n.n_theta, n.g_off, p.n_acc, p.n_weights);
        printf("\"net\": \"%d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %d, %uu, %uu, %uu, %uu, %uu\", \"leaves\": [", n.P, n.K, n.G, n.T, n.F, n.n_theta, n.g_off, n.scale_nn, n.mech,
               n.n_par, n.loss, n.n_out, n.targ_out, n.par_kind, n.par_idx, n.forc_col, n.loss_t);
        for (size_t i = 0; i < p.leaves.size(); ++i) {
            const EhLeaf& l = p.leaves[i];
            printf("%s[%d, %d, \"%s\", %d, %d, %d, %s]", i ? ", " : "", l.net, l.layer, eh_leaf_name(l.kind), l.off, l.rows, l.cols, l.is_weight ? "true" : "false");
        }
        printf("], \"norm\": {\"total\": %d, \"widest\": %d, \"layers\": [", p.bnl_tot, p.norm_maxn);      // BatchNorm layers: [layer, offset of its running statistics, width]
        bool first = true;
        for (int l = 0; l < p.l_net[0].nl; ++l)
            if (eh_is_norm(p.l_net[0].kind[l]) && !eh_is_layernorm(p.l_net[0].kind[l])) { printf("%s[%d, %d, %d]", first ? "" : ", ", l, p.bnl_off[l], p.l_net[0].out[l]); first = false; }
        printf("]}}\n");
    }
    fclose(f);
    return 0;
}
