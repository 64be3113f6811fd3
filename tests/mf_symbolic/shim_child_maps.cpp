// TEST INFRASTRUCTURE (host only): shim.cpp plus the arrays of the launch plan that the tile kernels of the extend-add read (child row maps, child records,
// tile records), for tests/test_mf_child_maps.py.  One translation unit with shim.cpp, so that both see the same analysis and plan.  Built by the test with g++.
#include "shim.cpp"

extern "C" long long shim_plan_fetch_maps(const char* name, long long* out)
{
    const std::string n = name;
    std::vector<long long> v;
    const MfPlan& p = g_plan;
    if (n == "childMap") v.assign(p.childMap.begin(), p.childMap.end());
    else if (n == "kidBase") v.assign(p.kidBase.begin(), p.kidBase.end());
    else if (n == "eaTile") v.assign(p.eaTile.begin(), p.eaTile.end());
    else if (n == "schurTile") v.assign(p.schurTile.begin(), p.schurTile.end());
    else if (n == "kidRec")
        for (const MfRec4& r : p.kidRec) v.insert(v.end(), { r.x, r.y, r.z, r.w });
    else if (n == "schurTileOff")
        for (const MfLevelPlan& P : p.level) v.push_back(P.schurTileOff);
    else if (n == "geometry") v = { TILE_REC, TILE_MAP_PAD };
    else return -1;
    if (out) std::copy(v.begin(), v.end(), out);
    return (long long)v.size();
}
