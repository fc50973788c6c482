// Host program of tests/test_loop_deal.py: csrc/loop_deal.h as the compiler of the host sees it.  Prints, one line per
// (nw, slot): "nw slot table0..3 formula0..3" — what loop_deal_unit and the formula return for the SIMDs 0..3.
#include <cstdio>

#include "loop_deal.h"

int main() {
    using namespace sageicp::loopdeal;
    static_assert(kTableFirstSlot == 4 && kTableSlots == 6, "slots 4-9 come from the table");
    for (unsigned nw = 1; nw <= 8; ++nw)
        for (unsigned slot = 0; slot < 16; ++slot) {
            std::printf("%u %u", nw, slot);
            for (unsigned s = 0; s < 4; ++s) std::printf(" %u", loop_deal_unit(s, slot, nw));
            for (unsigned s = 0; s < 4; ++s) std::printf(" %u", formula(s, slot, nw));
            std::printf("\n");
        }
    return 0;
}
