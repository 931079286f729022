// Stand-alone proof of the JPEG encoder's quantiser (rtm3d_amd/csrc/jpeg_quant.h, the function the device stage compiles):
// for every table entry q = 1..255 and every |c| = 0..32767, both signs, jpeg_quantise equals the rule
// a = (|c| + 4 q) / (8 q) truncating, c < 0 ? -a : a.  255 * 32768 * 2 cases.  Exit status 0 and a line of counts, or 1 and the
// first mismatch.
#include <stdint.h>
#include <stdio.h>

#include "../rtm3d_amd/csrc/jpeg_quant.h"

int main() {
    unsigned long long cases = 0;
    for (uint32_t q = 1; q <= 255; ++q) {
        const uint32_t m = jpeg_quant_multiplier(q);
        for (int32_t a = 0; a <= 32767; ++a) {
            const int32_t want = (int32_t)(((uint32_t)a + 4u * q) / (8u * q));
            const int32_t pos = jpeg_quantise(a, q, m), neg = jpeg_quantise(-a, q, m);
            if (pos != want || neg != -want) {
                printf("q %u c %d: got %d / %d, the rule gives %d / %d\n", q, a, pos, neg, want, -want);
                return 1;
            }
            cases += 2;
        }
    }
    printf("%llu cases, no mismatch\n", cases);
    return 0;
}
