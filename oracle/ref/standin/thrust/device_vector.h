// Stand-in for <thrust/device_vector.h>: device pointers are host pointers.
#pragma once
#include <algorithm>

namespace thrust
{
template <typename T> class device_ptr
{
public:
  explicit device_ptr(T *p = nullptr) : m_p(p) {}
  T *get() const { return m_p; }
  device_ptr operator+(std::ptrdiff_t n) const { return device_ptr(m_p + n); }
private:
  T *m_p;
};
template <typename T> device_ptr<T> device_pointer_cast(T *p) { return device_ptr<T>(p); }
template <typename T> void fill(device_ptr<T> first, device_ptr<T> last, const T &v) { std::fill(first.get(), last.get(), v); }
}
