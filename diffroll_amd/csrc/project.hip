// gfx950 (MI355X, CDNA4): options "cfg_project" / "cfg_norm" - the statistics behind adaptive projected guidance (Sadat et al.
// 2024, "Eliminating Oversaturation and Artifacts of High Guidance Scales in Diffusion Models"), without its momentum.
// Per GROUP (kernels.h: ProjectArgs - a clip's roll, or a recording's canvas) the launch here leaves
//   a = (float)((1 - s) - s (rho k)),  b = (float)s,   k = Scd / Scc,  s = min(1, r / (sqrt(Sdd / N) / |w|))
// in the group's record: the sums over the conditional prediction c and d = y - c of the guided prediction y, in the fixed
// order and by the two launch forms of group_sums.h ("cfg_rescale"'s).  Here: the statistic, its two kernels and launcher.
#include "project_quad.h"
#include "group_sums.h"

namespace dr {
#pragma clang fp contract(off)

struct ProjectStat {
    static constexpr int K = PROJECT_SUMS;
    using Args = ProjectArgs;
    __host__ __device__ static inline const UpdateArgs& u(const Args& a) { return a.u; }
    __host__ __device__ static inline unsigned* work(const Args& a) { return a.work; }
    static DR_DEVINL void frame(const Args& a, const UpdateArgs& uc, const long row, const int f, double (&s)[K]) {
        project_frame(a.u, uc, row, f, s, PlainY{});
    }
    static DR_DEVINL void record(const Args& a, const long row, const double N, const double (&s)[K]) { project_record(a, row, N, s); }
};

__global__ __launch_bounds__(256) void project_roll_kernel(const ProjectArgs a) { gs_roll<ProjectStat>(a); }
__global__ __launch_bounds__(64) void project_grid_kernel(const ProjectArgs a) { gs_grid<ProjectStat>(a); }

hipError_t launch_project(const ProjectArgs& a, int B, hipStream_t s) {
    if (a.rho < 0 || a.rho > 10000 || a.norm < 0 || a.norm > 100000 || (a.rho == 0 && a.norm == 0)) return hipErrorInvalidValue;
    return gs_launch<ProjectStat>(project_roll_kernel, project_grid_kernel, a, B, s);
}

}  // namespace dr
