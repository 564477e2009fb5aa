// polygon.h -- the integer point-in-polygon test shared by the zone engine (zones.hip) and the renderer's zone tint
// (render.hip), so that the tinted area is exactly the area where the zone engine fires.
#pragma once

#include <hip/hip_runtime.h>

namespace rtmodt {

// cv::pointPolygonTest(contour int32, integer point, measureDist=false) >= 0  (oracle/zone_oracle.py:point_polygon_test)
__device__ __forceinline__ bool inside_or_on(const int2 *p, int total, int x, int y) {
    if (total == 0) return false;
    int counter = 0;
    int2 v = p[total - 1];
    for (int i = 0; i < total; ++i) {
        const int2 v0 = v;
        v = p[i];
        if ((v0.y <= y && v.y <= y) || (v0.y > y && v.y > y) || (v0.x < x && v.x < x)) {
            if (y == v.y && (x == v.x || (y == v0.y && ((v0.x <= x && x <= v.x) || (v.x <= x && x <= v0.x))))) return true;
            continue;
        }
        long long dist = (long long)(y - v0.y) * (v.x - v0.x) - (long long)(x - v0.x) * (v.y - v0.y);
        if (dist == 0) return true;
        if (v.y < v0.y) dist = -dist;
        counter += dist > 0;
    }
    return (counter & 1) != 0;
}

}  // namespace rtmodt
