// The element conversions of weight_image_kernel (memex_amd/csrc/mx_weight_forms.h), compiled for the host and compared with
// the library's host routines through mx_encoder_weight_image(via_device = 0): every 997th f32 bit pattern plus the
// neighbourhoods of the values where a rounding, a saturation or a NaN rule changes.  No GPU.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/memex_hip.h"
#include "../../memex_amd/csrc/mx_weight_forms.h"

int main() {
    std::vector<uint32_t> bits;
    for (uint64_t u = 0; u < (1ull << 32); u += 997) bits.push_back((uint32_t)u);
    const uint32_t centres[] = {0x00000000u, 0x00800000u, 0x33000000u, 0x33800000u, 0x38800000u, 0x387fc000u, 0x477fe000u, 0x477ff000u,
                                0x47800000u, 0x7f7fffffu, 0x7f800000u, 0x7fc00000u, 0x7f7f8000u, 0x3f808000u, 0x3f818000u, 0x3c001000u,
                                0x3c003000u, 0x33c00000u, 0x36a00000u};
    for (uint32_t c : centres)
        for (int d = -70; d <= 70; ++d)
            for (uint32_t sign : {0u, 0x80000000u}) bits.push_back((c + (uint32_t)d) ^ sign);
    const int k = 1024;
    while (bits.size() % k) bits.push_back(0x3d4ccccdu);
    const int rows = (int)(bits.size() / k);
    std::vector<float> w(bits.size());
    memcpy(w.data(), bits.data(), bits.size() * 4);
    long bad = 0;
    for (int form : {MX_PREC_BF16, MX_PREC_BF16X3, MX_PREC_MIXED, MX_PREC_MIXED1}) {
        const size_t copies = form == MX_PREC_BF16X3 ? 3 : form == MX_PREC_MIXED ? 2 : 1;
        std::vector<uint16_t> img((size_t)rows * k * copies);
        if (mx_encoder_weight_image(w.data(), rows, k, form, 0, 0, img.data()) != MX_OK) {
            printf("mx_encoder_weight_image failed: %s\n", mx_last_error());
            return 1;
        }
        auto at = [&](size_t r, size_t c) { return img[((c >> 5) * rows + r) * 32 + (c & 31)]; };
        for (size_t r = 0; r < (size_t)rows; ++r)
            for (size_t c = 0; c < (size_t)k; ++c) {
                const uint32_t u = bits[r * k + c];
                uint16_t want[3];
                if (form == MX_PREC_BF16 || form == MX_PREC_BF16X3) {
                    want[0] = want[1] = mx::wf_bf16(u);
                    want[2] = mx::wf_bf16_lo(u, want[0]);
                } else {
                    want[0] = want[1] = mx::wf_f16_sat(u);
                }
                for (size_t j = 0; j < copies; ++j)
                    if (at(r, j * k + c) != want[j] && bad++ < 20)
                        printf("form %d copy %zu: f32 %08x -> host %04x, header %04x\n", form, j, u, at(r, j * k + c), want[j]);
            }
    }
    if (bad) {
        printf("FAILED: %ld mismatches\n", bad);
        return 1;
    }
    printf("OK weight forms (%zu values)\n", bits.size());
    return 0;
}
