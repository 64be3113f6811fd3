// Stand-alone driver of ipc_amd/csrc/round_collider_plan.cpp for tests/test_round_collider_plan_host.py.  One collider per input line:
//   p0x p0y p0z p1x p1y p1z R hollow dHat          (hexadecimal or decimal floats, "nan" / "inf" included)
// and one output line each: "1 p0[3] p1[3] axis[3] len R side" in hexadecimal floats, or "0 <reason>".
#include "round_collider_plan.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <sstream>
#include <string>

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string tok[9];
        for (auto& t : tok)
            if (!(in >> t)) return 2;
        double v[9];
        for (int i = 0; i < 9; ++i) v[i] = std::strtod(tok[i].c_str(), nullptr);
        ipcgpu::RoundShape s;
        std::string err;
        if (!ipcgpu::planRoundCollider(v, v + 3, v[6], (int)v[7], v[8], s, err)) {
            std::printf("0 %s\n", err.c_str());
            continue;
        }
        std::printf("1");
        for (double q : s.p0) std::printf(" %a", q);
        for (double q : s.p1) std::printf(" %a", q);
        for (double q : s.axis) std::printf(" %a", q);
        std::printf(" %a %a %a\n", s.len, s.R, s.side);
        if (v[8] > 0.0 && !ipcgpu::checkRoundColliderDHat(s, v[8], err)) return 3; // (planRoundCollider asked already)
    }
    return 0;
}
