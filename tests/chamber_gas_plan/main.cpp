// Stand-alone driver of the gas part of ipc_amd/csrc/chamber_plan.cpp (buildChamberGas, chamberGasPressureOk) for tests/test_chamber_gas_plan_host.py
// (plain g++, once more under the sanitizers).  The plan it works on is given by its numbers: no geometry is needed for the slices.
// stdin, per set:   nCh hasFill | nCh triEnd | nCh pressures | nCh rest volumes | nCh x (isGas ambient gamma fill) | nCh new pressures
//                   (numbers are read with strtod: "nan" and "inf" are numbers here; hasFill == 0 hands a null fill-volume pointer)
// stdout, per set:  "0 <reason>" or
//   "1 nGas nSlice <0 / 1: the new pressures are accepted> | nGas gas chambers | nGas + 1 sliceOff | nSlice begin | nSlice end | nCh fill volumes"
#include "chamber_plan.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>

static double number(std::istream& in)
{
    std::string tok;
    in >> tok;
    return std::strtod(tok.c_str(), nullptr);
}

int main()
{
    int nCh, hasFill;
    while (std::cin >> nCh >> hasFill) {
        const size_t n = (size_t)(nCh > 0 ? nCh : 0);
        ipcgpu::ChamberPlan plan;
        plan.n = nCh;
        plan.triEnd.resize(n);
        plan.pressure.resize(n);
        plan.restVolume.resize(n);
        for (size_t c = 0; c < n; ++c) std::cin >> plan.triEnd[c];
        for (size_t c = 0; c < n; ++c) plan.pressure[c] = number(std::cin);
        for (size_t c = 0; c < n; ++c) plan.restVolume[c] = number(std::cin);
        plan.nTri = n ? plan.triEnd[n - 1] : 0;
        std::vector<int> isGas(n);
        std::vector<double> ambient(n), gamma(n), fill(n), next(n);
        for (size_t c = 0; c < n; ++c) {
            std::cin >> isGas[c];
            ambient[c] = number(std::cin);
            gamma[c] = number(std::cin);
            fill[c] = number(std::cin);
        }
        for (size_t c = 0; c < n; ++c) next[c] = number(std::cin);
        ipcgpu::ChamberGas gas;
        std::string err;
        if (!ipcgpu::buildChamberGas(plan, isGas.data(), ambient.data(), gamma.data(), hasFill ? fill.data() : nullptr, gas, err)) {
            std::printf("0 %s\n", err.c_str());
            continue;
        }
        std::string perr;
        std::printf("1 %d %d %d", gas.nGas, gas.nSlice(), ipcgpu::chamberGasPressureOk(gas, nCh, next.data(), perr) ? 1 : 0);
        for (int v : gas.gasChamber) std::printf(" %d", v);
        for (int v : gas.sliceOff) std::printf(" %d", v);
        for (int v : gas.sliceBegin) std::printf(" %d", v);
        for (int v : gas.sliceEnd) std::printf(" %d", v);
        for (double v : gas.fillVolume) std::printf(" %.17g", v);
        std::printf("\n");
    }
    return 0;
}
