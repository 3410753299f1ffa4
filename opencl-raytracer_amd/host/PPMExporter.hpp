// PPMExporter.hpp - ASCII PPM sink with the reference's signature (PPMExporter.hpp:8) and byte-for-byte output
// (PPMExporter.cpp:13-23): "P3\n<w> <h>\n255\n", then per pixel `min(255, (int)floorf(v * 255.f))` for r, g, b
// separated by single spaces, one pixel per line. RGBAtoRGB repacks Render()'s float4 frame to the packed
// stride-3 vector ExportP3 expects. The overloads that take bytes write a frame that already is 8 bits per channel
// (HIPRaytracer::RenderPacked): `stride` bytes per pixel, 3 (RGB8) or 4 (RGBA8, the fourth byte is skipped); ExportP6 is the
// binary flavour ("P6\n<w> <h>\n255\n", then 3 bytes per pixel).
#pragma once

#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

class PPMExporter {
public:
    static void ExportP3(const std::string& outFileLoc, size_t width, size_t height, const std::vector<float>& pixelData);
    static void ExportP3(const std::string& outFileLoc, size_t width, size_t height, const uint8_t* pixels, size_t stride);
    static void ExportP6(const std::string& outFileLoc, size_t width, size_t height, const uint8_t* pixels, size_t stride);
    static std::vector<float> RGBAtoRGB(const float* rgba, size_t pixels);
};
