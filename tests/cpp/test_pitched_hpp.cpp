// include/hgi.hpp, Encoder::encode_view / Decoder::decode_view on a device: the window of a parent image encoded where it lies
// equals encode() of its packed copy, and decode_view into a window of a sentinel-filled canvas equals decode() and leaves the
// canvas elsewhere untouched.  Prints "ok" and exits 0.  (Built and run by tests/test_pitched_gpu.py.)
#include <cstdio>
#include <cstring>
#include <vector>

#include "hgi.hpp"

using namespace hgi;

int main()
{
    const uint32_t PW = 517, PH = 301, X = 13, Y = 7, W = 403, H = 255;
    std::vector<uint8_t> parent((size_t)PW * PH);
    uint32_t x = 12345;
    for (auto &v : parent) v = (uint8_t)((x = x * 1664525u + 1013904223u) >> 24);
    for (size_t levels : {3, 7, 9}) {
        Encoder<interpolator::Crossed, quantizator::Linear> enc(interpolator::Crossed{}, quantizator::Linear::from(quantizator::QuantizationLevel::Medium), levels);
        Decoder<interpolator::Crossed> dec(interpolator::Crossed{});
        GrayImage crop(W, H);
        for (uint32_t r = 0; r < H; ++r) std::memcpy(crop.data.data() + (size_t)r * W, parent.data() + (size_t)(Y + r) * PW + X, W);
        const Grid a = enc.encode_view(parent.data() + (size_t)Y * PW + X, PW, W, H), b = enc.encode(crop);
        if (!(a == b)) return std::printf("levels %zu: encode_view differs from encode\n", levels), 1;
        std::vector<uint8_t> canvas((size_t)PW * PH, 0xC3);
        dec.decode_view({W, H}, levels, a, canvas.data() + (size_t)Y * PW + X, PW);
        const GrayImage want = dec.decode({W, H}, levels, a);
        for (uint32_t r = 0; r < PH; ++r)
            for (uint32_t c = 0; c < PW; ++c) {
                const bool in = r >= Y && r < Y + H && c >= X && c < X + W;
                const uint8_t v = canvas[(size_t)r * PW + c], w = in ? want.data[(size_t)(r - Y) * W + (c - X)] : (uint8_t)0xC3;
                if (v != w) return std::printf("levels %zu: canvas (%u, %u) = %u, want %u\n", levels, c, r, v, w), 1;
            }
    }
    std::printf("ok\n");
    return 0;
}
