// conv_plan.cpp -- see conv_plan.hpp.
#include "conv_plan.hpp"

#include "common.hpp"

#include <algorithm>
#include <utility>

namespace ecm2
{

ConvPlan build_conv_plan(const std::vector<int> &gather_map, int ne, int nd, int ndofs,
                         const std::vector<unsigned char> &keep, bool blocked)
{
   ECM2_VERIFY(ne >= 0 && nd > 0 && ndofs >= 0, ERR_ARG, "convection plan sizes");
   ECM2_VERIFY(gather_map.size() == (size_t)ne * nd && keep.size() == (size_t)ne, ERR_ARG,
               "convection plan: map or marker size");
   ConvPlan p;
   p.blocked = blocked ? 1 : 0;
   for (int e = 0; e < ne; e++)
   {
      if (keep[e]) { p.act.push_back(e); }
   }
   p.n_act = (int)p.act.size();
   const int nblk = (p.n_act + kConvBlock - 1) / kConvBlock;
   p.ev_size = blocked ? (size_t)nblk * nd * kConvBlock : (size_t)p.n_act * nd;
   ECM2_VERIFY(p.ev_size < ((size_t)1 << 31), ERR_UNSUPPORTED, "convection E-vector of " << p.ev_size << " entries");
   p.map.assign(p.ev_size, 0);
   // (dof, k nd + i): sorted, a dof's entries ascend in element then local index
   std::vector<std::pair<int, long>> ent;
   ent.reserve((size_t)p.n_act * nd);
   for (int k = 0; k < p.n_act; k++)
   {
      const int *row = gather_map.data() + (size_t)p.act[k] * nd;
      for (int i = 0; i < nd; i++)
      {
         const int g = row[i], d = g >= 0 ? g : -1 - g;
         ECM2_VERIFY(d >= 0 && d < ndofs, ERR_ARG, "gather map entry " << g << " out of range [0," << ndofs << ")");
         p.map[conv_ev_index(blocked, nd, k, i)] = g;
         ent.emplace_back(d, (long)k * nd + i);
      }
   }
   if (blocked)
   {
      // the padding lanes of the last block read what its first lane reads
      for (int k = p.n_act; k < nblk * kConvBlock; k++)
         for (int i = 0; i < nd; i++)
         {
            p.map[conv_ev_index(true, nd, k, i)] = p.map[conv_ev_index(true, nd, (k / kConvBlock) * kConvBlock, i)];
         }
   }
   std::sort(ent.begin(), ent.end());
   p.csr_idx.resize(ent.size());
   for (size_t j = 0; j < ent.size(); j++)
   {
      if (j == 0 || ent[j].first != ent[j - 1].first)
      {
         p.csr_dof.push_back(ent[j].first);
         p.csr_off.push_back((int)j);
      }
      const int k = (int)(ent[j].second / nd), i = (int)(ent[j].second % nd);
      const long pos = (long)conv_ev_index(blocked, nd, k, i);
      const bool neg = gather_map[(size_t)p.act[k] * nd + i] < 0;
      p.csr_idx[j] = neg ? (int)(-1 - pos) : (int)pos;
   }
   p.csr_off.push_back((int)ent.size());
   p.n_rows = (int)p.csr_dof.size();
   return p;
}

} // namespace ecm2
