// Stand-in for NGL's ngl::Vec3 (the NCCA graphics library): three floats
// readable by name or as an array, with the arithmetic a bounding-volume
// builder needs.  Plain IEEE float operations, one per operator.
#pragma once

namespace ngl
{
class Vec3
{
public:
  Vec3() : m_x(0.f), m_y(0.f), m_z(0.f) {}
  Vec3(float _x, float _y, float _z) : m_x(_x), m_y(_y), m_z(_z) {}
  Vec3 operator+(const Vec3 &_v) const { return Vec3(m_x + _v.m_x, m_y + _v.m_y, m_z + _v.m_z); }
  Vec3 operator-(const Vec3 &_v) const { return Vec3(m_x - _v.m_x, m_y - _v.m_y, m_z - _v.m_z); }
  Vec3 operator*(float _s) const { return Vec3(m_x * _s, m_y * _s, m_z * _s); }
  Vec3 operator/(float _s) const { return Vec3(m_x / _s, m_y / _s, m_z / _s); }
  Vec3 &operator+=(const Vec3 &_v) { m_x += _v.m_x; m_y += _v.m_y; m_z += _v.m_z; return *this; }
  Vec3 &operator-=(const Vec3 &_v) { m_x -= _v.m_x; m_y -= _v.m_y; m_z -= _v.m_z; return *this; }
  Vec3 &operator*=(float _s) { m_x *= _s; m_y *= _s; m_z *= _s; return *this; }
  Vec3 &operator/=(float _s) { m_x /= _s; m_y /= _s; m_z /= _s; return *this; }
  float &operator[](int _i) { return m_openGL[_i]; }
  const float &operator[](int _i) const { return m_openGL[_i]; }
  union
  {
    struct
    {
      float m_x, m_y, m_z;
    };
    float m_openGL[3];
  };
};
inline Vec3 operator*(float _s, const Vec3 &_v) { return _v * _s; }
}
