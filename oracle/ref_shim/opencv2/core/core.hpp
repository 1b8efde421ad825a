// TEST INFRASTRUCTURE — a stand-in for <opencv2/core/core.hpp>, this project's own text, so that the
// reference's DBoW2 sources compile without OpenCV (oracle/Makefile target `ref`).  DBoW2 uses cv::Mat
// only as a row of bytes (create, zeros, clone, release, ptr<T>(), rows, cols, empty) and only names
// cv::FileStorage / cv::FileNode (the YAML load/save, never called by the driver).
//
// Differences from OpenCV, on purpose:
//  * Mat::create ZERO-FILLS a new buffer.  Real OpenCV leaves the memory uninitialised, so a
//    descriptor that FORB::fromString does not write (the loader's trailing-newline node, DESIGN.md
//    Q21) is indeterminate there and 32 zero bytes here.
//  * FileStorage never opens: isOpened() is false, writes are dropped, reads give empty nodes.
// DBoW2 relies on OpenCV pulling in the C math / stdlib names and the stream headers; so does this.
#pragma once
#include <math.h>
#include <stdlib.h>
#include <cstddef>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>

#define CV_8U 0
#define CV_32F 5

namespace cv {

class Mat {
public:
    int rows = 0, cols = 0;

    Mat() {}
    // copies share the buffer, as cv::Mat headers do
    void create(int r, int c, int type) {
        const size_t esz = type == CV_32F ? 4 : 1;
        if (buf_ && r == rows && c == cols && esz == esz_) return;
        rows = r;
        cols = c;
        esz_ = esz;
        const size_t n = (size_t)r * (size_t)c * esz;
        buf_.reset(new unsigned char[n ? n : 1], std::default_delete<unsigned char[]>());
        std::memset(buf_.get(), 0, n);  // zero-filled: see the header comment
    }
    static Mat zeros(int r, int c, int type) {
        Mat m;
        m.create(r, c, type);
        return m;
    }
    Mat clone() const {
        Mat m;
        if (buf_) {
            m.create(rows, cols, esz_ == 4 ? CV_32F : CV_8U);
            std::memcpy(m.buf_.get(), buf_.get(), (size_t)rows * (size_t)cols * esz_);
        }
        return m;
    }
    void release() {
        buf_.reset();
        rows = cols = 0;
    }
    bool empty() const { return !buf_ || rows == 0 || cols == 0; }
    template <class T> T* ptr(int row = 0) { return reinterpret_cast<T*>(buf_.get() + (size_t)row * cols * esz_); }
    template <class T> const T* ptr(int row = 0) const {
        return reinterpret_cast<const T*>(buf_.get() + (size_t)row * cols * esz_);
    }

private:
    std::shared_ptr<unsigned char> buf_;
    size_t esz_ = 1;
};

class FileNode {
public:
    FileNode operator[](const char*) const { return FileNode(); }
    FileNode operator[](const std::string&) const { return FileNode(); }
    FileNode operator[](int) const { return FileNode(); }
    size_t size() const { return 0; }
    operator int() const { return 0; }
    operator double() const { return 0.0; }
    operator std::string() const { return std::string(); }
};

class FileStorage {
public:
    enum { READ = 0, WRITE = 1 };
    FileStorage() {}
    FileStorage(const std::string&, int) {}
    bool isOpened() const { return false; }
    FileNode operator[](const char*) const { return FileNode(); }
    FileNode operator[](const std::string&) const { return FileNode(); }
};

template <class T> inline FileStorage& operator<<(FileStorage& fs, const T&) { return fs; }

}  // namespace cv
