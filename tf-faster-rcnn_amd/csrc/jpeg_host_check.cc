// Stand-alone sanitizer harness for csrc/jpeg_host.h (not part of libfrcnn_hip.so):
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all -I include -I tf-faster-rcnn_amd/csrc \
//       tf-faster-rcnn_amd/csrc/jpeg_host_check.cc -o jpeg_host_check && ./jpeg_host_check a.jpg b.jpg ...
// Every file is decoded whole, at every truncation length in steps of 7 bytes and with 300 seeded single-byte corruptions; the input and
// the coefficient buffer are heap blocks of exactly the sizes handed over, so a read or write one byte outside either is reported.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "jpeg_host.h"

static int run(const unsigned char* d, size_t n, size_t coef_bytes, int* counts) {
  unsigned char* in = (unsigned char*)malloc(n ? n : 1);
  memcpy(in, d, n);
  unsigned char* coef = (unsigned char*)malloc(coef_bytes);
  int info[8];
  const int ri = jpeg_host::info(in, n, info);
  const int rc = jpeg_host::entropy_decode(in, n, coef, coef_bytes);
  if (rc == FRCNN_OK) {
    JpegGeom g;
    if (ri != FRCNN_OK || !jpeg_geom(info[0], info[1], info[2], info[3], info[4], &g) || g.coef_bytes > coef_bytes) abort();
    std::vector<unsigned char> planes(g.ws_bytes), bgr((size_t)g.w * g.h * 3);
    jpeg_host::pixels_host(coef, g, planes.data(), bgr.data());
  }
  if (rc != FRCNN_OK && rc != FRCNN_E_ARG && rc != FRCNN_E_UNSUPPORTED) abort();
  ++counts[rc == FRCNN_OK ? 0 : (rc == FRCNN_E_ARG ? 1 : 2)];
  free(coef);
  free(in);
  return rc;
}

int main(int argc, char** argv) {
  int counts[3] = {0, 0, 0};
  for (int a = 1; a < argc; ++a) {
    FILE* f = fopen(argv[a], "rb");
    if (!f) return 2;
    std::vector<unsigned char> d;
    for (int c; (c = fgetc(f)) != EOF;) d.push_back((unsigned char)c);
    fclose(f);
    int info[8];
    if (jpeg_host::info(d.data(), d.size(), info) != FRCNN_OK) return 3;
    JpegGeom g;
    jpeg_geom(info[0], info[1], info[2], info[3], info[4], &g);
    if (run(d.data(), d.size(), g.coef_bytes, counts) != FRCNN_OK) return 4;
    for (size_t cut = 0; cut < d.size(); cut += 7) run(d.data(), cut, g.coef_bytes, counts);
    unsigned s = 12345u + (unsigned)a;
    for (int i = 0; i < 300; ++i) {
      std::vector<unsigned char> m(d);
      s = s * 1664525u + 1013904223u;
      const size_t at = 2 + (s >> 8) % (m.size() - 2);
      s = s * 1664525u + 1013904223u;
      m[at] = (unsigned char)(s >> 16);
      run(m.data(), m.size(), g.coef_bytes, counts);
    }
  }
  printf("ok %d, damaged %d, unsupported %d\n", counts[0], counts[1], counts[2]);
  return 0;
}
