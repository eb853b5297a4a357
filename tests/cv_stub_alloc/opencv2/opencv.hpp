// TEST-ONLY layer in front of tests/cv_stub (put -Itests/cv_stub_alloc BEFORE -Itests/cv_stub): the stand-in of cv::Mat there has
// no allocator, so this header takes it in under another name and derives a cv::Mat that allocates through cv::MatAllocator /
// cv::UMatData with the members ms-slam_amd/host/PinnedMat.h uses (the shape of OpenCV 4's public declarations in core/mat.hpp,
// nothing of its implementation).  Reference-counted like the real one: copies share the block, the last one gives it back to
// the allocator that made it.  Never used to build reference sources.
#pragma once
#define Mat StubMat
#include_next <opencv2/opencv.hpp>
#undef Mat
#include <cstdlib>

#define CV_ELEM_SIZE(type) ((size_t)1)   // (the stand-in knows CV_8UC1 only)

namespace cv {
enum AccessFlag { ACCESS_READ = 1 << 24, ACCESS_WRITE = 1 << 25, ACCESS_RW = 3 << 24 };
enum UMatUsageFlags { USAGE_DEFAULT = 0 };
struct UMatData;
class MatAllocator {
public:
    MatAllocator() {}
    virtual ~MatAllocator() {}
    virtual UMatData* allocate(int dims, const int* sizes, int type, void* data, size_t* step, AccessFlag flags, UMatUsageFlags usageFlags) const = 0;
    virtual bool allocate(UMatData* data, AccessFlag accessflags, UMatUsageFlags usageFlags) const = 0;
    virtual void deallocate(UMatData* data) const = 0;
};
struct UMatData {
    enum MemoryFlag { USER_ALLOCATED = 32 };
    explicit UMatData(const MatAllocator* allocator) : prevAllocator(allocator), currAllocator(allocator) {}
    const MatAllocator* prevAllocator;
    const MatAllocator* currAllocator;
    int urefcount = 0, refcount = 0;
    unsigned char* data = nullptr;
    unsigned char* origdata = nullptr;
    size_t size = 0;
    int flags = 0;
};

class Mat : public StubMat {
public:
    UMatData* u = nullptr;
    Mat() {}
    Mat(int r, int c, int t, void* d, size_t s) : StubMat(r, c, t, d, s) {}
    Mat(const StubMat& m) : StubMat(m) { if (!own.empty()) data = own.data(); }
    Mat(const Mat& m) : StubMat(static_cast<const StubMat&>(m)), u(m.u) { if (u) u->refcount++; if (!own.empty()) data = own.data(); }
    Mat& operator=(const Mat& m) {
        if (this == &m) return *this;
        if (m.u) m.u->refcount++;
        release();
        StubMat::operator=(static_cast<const StubMat&>(m));
        if (!own.empty()) data = own.data();
        u = m.u;
        return *this;
    }
    ~Mat() { release(); }
    void release() {
        if (u && --u->refcount == 0) u->currAllocator->deallocate(u);
        u = nullptr;
        StubMat::release();
    }
    void create(int r, int c, int t) {
        release();
        const int sizes[2] = {r, c};
        size_t st[2] = {0, 0};
        u = getDefaultAllocator()->allocate(2, sizes, t, nullptr, st, ACCESS_RW, USAGE_DEFAULT);
        u->refcount = 1;
        rows = r; cols = c; step = st[0]; data = u->data;
    }
    Mat clone() const {
        Mat m;
        m.create(rows, cols, type());
        for (int y = 0; y < rows; y++) std::memcpy(m.data + (size_t)y * m.step, data + (size_t)y * step, (size_t)cols);
        return m;
    }
    static MatAllocator* getStdAllocator() {
        class Std : public MatAllocator {
        public:
            UMatData* allocate(int dims, const int* sizes, int type, void* data0, size_t* step, AccessFlag, UMatUsageFlags) const override {
                size_t total = CV_ELEM_SIZE(type);
                for (int i = dims - 1; i >= 0; i--) {
                    if (step) step[i] = total;
                    total *= (size_t)sizes[i];
                }
                UMatData* d = new UMatData(this);
                d->data = d->origdata = data0 ? static_cast<unsigned char*>(data0) : static_cast<unsigned char*>(std::malloc(total ? total : 1));
                d->size = total;
                if (data0) d->flags |= UMatData::USER_ALLOCATED;
                return d;
            }
            bool allocate(UMatData* d, AccessFlag, UMatUsageFlags) const override { return d != nullptr; }
            void deallocate(UMatData* d) const override {
                if (!d) return;
                if (!(d->flags & UMatData::USER_ALLOCATED)) std::free(d->origdata);
                delete d;
            }
        };
        static Std* const a = new Std();
        return a;
    }
    static MatAllocator*& default_slot() { static MatAllocator* a = getStdAllocator(); return a; }
    static MatAllocator* getDefaultAllocator() { return default_slot(); }
    static void setDefaultAllocator(MatAllocator* a) { default_slot() = a; }
};
}  // namespace cv
