// capi_common.cpp -- error string storage and version entry points of the C ABI.
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "fps_select.h"
#include "sn_common.h"

long long sn_emd_workspace_floats(int b, int n, int m);
long long sn_emd_loss_floats(int b, int n, int m);

static thread_local char g_err[512] = "";

int sn_set_error(int code, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

extern "C" int sn_abi_version(void) { return SN_ABI_VERSION; }
extern "C" const char *sn_last_error_string(void) { return g_err; }
extern "C" long long sn_workspace_bytes(const char *op, int B, int N, int M, int K)
{
    (void)K;
    if (!op) return -1;
    // approxmatch: the reference op allocates (b,(n+m)*2) floats (tf_approxmatch.cpp:167-168); this
    // implementation keeps the ratio vectors of all 10 levels so that `match` is written once.
    if (!strcmp(op, "approxmatch")) return sn_emd_workspace_floats(B, N, M) * 4;
    if (!strcmp(op, "matchcost")) return (long long)B * ((N + 255) / 256) * 4;  // per-workgroup partial sums
    if (!strcmp(op, "emd_loss"))  // level workspace + cost partials (+ padding to 16 bytes) + the one-sweep form's tile partials
        return sn_emd_loss_floats(B, N, M) * 4;
    // furthest_point_sample: the streaming path's running minima (B*N floats); 0 where the shape runs register-resident
    if (!strcmp(op, "furthest_point_sample")) return B > 0 && N > 0 && sn::fps_choose(B, N) == 3 ? (long long)B * N * 4 : 0;
    // retrieval_metrics (S, n, C, L): a query's keys are sorted in its workgroup's LDS
    if (!strcmp(op, "retrieval_metrics")) return 0;
    return 0;
}

// the farthest-point sampling variant hook lives here, next to the workspace query that reads it, so that a library linked
// without sampling.o still resolves every symbol of this unit
int sn::g_fps_variant = 0;
extern "C" int sn_fps_set_variant(int v)
{
    const int prev = sn::g_fps_variant;
    if (v < 0 || v > 3) return -1;
    sn::g_fps_variant = v;
    return prev;
}
