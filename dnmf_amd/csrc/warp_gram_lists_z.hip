// K3n, the Z >= 2 instantiations (warp_gram_lists.hpp has the kernel, warp_gram_lists.hip the reasons and the Z == 1
// instantiations).  A translation unit of their own for build time only: this one compiles in about 50 s, the other in
// about 23 s, side by side; the flags are the same (dnmf_amd/build.py: PER_FILE_FLAGS).
#include "warp_gram_lists.hpp"

namespace dnmf {

void launch_lists_z(const ListParams &p, unsigned nwg, size_t lds, hipStream_t st, int nw) {
    if (p.vol.Z > 2) {
        if (nw == 1) launch_lists_t<3, 1>(p, nwg, lds, st);
        else if (nw == 2) launch_lists_t<3, 2>(p, nwg, lds, st);
        else launch_lists_t<3, 4>(p, nwg, lds, st);
    } else {
        if (nw == 1) launch_lists_t<2, 1>(p, nwg, lds, st);
        else if (nw == 2) launch_lists_t<2, 2>(p, nwg, lds, st);
        else launch_lists_t<2, 4>(p, nwg, lds, st);
    }
}

}  // namespace dnmf
