// The one-line integration of ms-slam_amd/host/PinnedMat.h, exercised the way System::TrackStereo feeds the extractor
// (System.cc:200-217): the application's image lies in pageable memory, the Mat that reaches ORBextractor::operator() is a fresh
// clone() — which, with msorb_host::PinnedMatAllocator installed as OpenCV's default allocator, lies in admitted pinned memory and
// is read in place by the unchanged drop-in class.  Compiled against tests/cv_stub_alloc layered in front of tests/cv_stub.
// usage: dropin_pinned <rows> <cols> <in.raw> <out.bin> <nfeatures>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "ORBextractor.h"
#include "PinnedMat.h"
#include "msorb.h"

int main(int argc, char** argv) {
    if (argc < 6) return 2;
    cv::Mat::setDefaultAllocator(msorb_host::PinnedMatAllocator::instance());   // the one line of INTEGRATION.md section 1
    const int rows = atoi(argv[1]), cols = atoi(argv[2]), nf = atoi(argv[5]);
    std::vector<unsigned char> buf((size_t)rows * cols);
    FILE* f = fopen(argv[3], "rb");
    if (!f || fread(buf.data(), 1, buf.size(), f) != buf.size()) return 3;
    fclose(f);
    ORB_SLAM3::ORBextractor* ex = new ORB_SLAM3::ORBextractor(nf, 1.2f, 8, 20, 7);   // Tracking.cc:595
    cv::Mat decoded(rows, cols, CV_8UC1, buf.data(), (size_t)cols), desc;   // what the application decoded: pageable
    std::vector<cv::KeyPoint> keys;
    std::vector<int> lap = {0, 0};
    int mono, admitted;
    const unsigned char* clone_data;
    {
        cv::Mat im = decoded.clone();   // System.cc:215-216
        clone_data = im.data;
        admitted = msorb_host_admitted(im.data, (size_t)(rows - 1) * im.step + cols);
        mono = (*ex)(im, cv::Mat(), keys, desc, lap);
    }   // the clone is released: its block is back in the pool ...
    cv::Mat next(rows, cols, CV_8UC1, buf.data(), (size_t)cols);
    cv::Mat reused = next.clone();   // ... and handed out again for the next frame,
    if (reused.data != clone_data) return 4;
    for (int y = 0; y < rows; y++) memset(reused.ptr<unsigned char>(y), 0x5a, cols);   // which overwrites it
    msorb_input_stats st;
    if (msorb_extractor_input_stats(ex->handle(), &st) != MSORB_OK) return 5;
    FILE* o = fopen(argv[4], "wb");
    const int n = (int)keys.size(), direct = (int)st.images_direct, staged = (int)st.images_staged;
    fwrite(&mono, 4, 1, o); fwrite(&n, 4, 1, o); fwrite(&direct, 4, 1, o); fwrite(&staged, 4, 1, o); fwrite(&admitted, 4, 1, o);
    fwrite(keys.data(), sizeof(cv::KeyPoint), n, o);
    for (int i = 0; i < n; i++) fwrite(desc.ptr<unsigned char>(i), 1, 32, o);
    for (int l = 0; l < ex->GetLevels(); l++) {   // mvImagePyramid stays readable: level 0 is the handle's copy, not the clone
        const cv::Mat& m = ex->mvImagePyramid[l];
        fwrite(&m.rows, 4, 1, o); fwrite(&m.cols, 4, 1, o);
        for (int y = 0; y < m.rows; y++) fwrite(m.ptr<unsigned char>(y), 1, m.cols, o);
    }
    fclose(o);
    delete ex;
    return 0;
}
